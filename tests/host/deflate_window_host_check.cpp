// Host check of csrc/vs_deflate_window_core.h: the logic of vs_deflate_chunks_window, compiled for the CPU (with sanitizers where they link)
// and run on a case file that tests/test_deflate_window_cpu.py writes.  Every chunk is compressed from an exactly-sized heap copy of its
// history + its bytes into an exactly-sized heap image, with exactly-sized per-position words, so that a read or a write outside any of
// them is a sanitizer report.  Checked here: the slot bound, that the chunk is never larger than vsd_deflate_chunk makes of the same bytes
// and IS those bytes when the runs parse is kept, that the kept form is the smallest by its own counts, and -- for a record without
// history -- that the chunks + a final block, framed as a zlib stream, inflate to the input through csrc/vs_inflate_core.h.
//
//   deflate_window_host_check CASES OUT CHUNK_BYTES
// CASES (little-endian): int64 records; per record int64 history, int64 n and history + n bytes (the history first).  Chunk c of a record
// sees min(32768, history + c * CHUNK_BYTES) bytes before it, as the kernel's chunk c does.
// OUT: int64 records; per record int64 bytes, int64 chunks, per chunk (int32 form, int32 bytes, int32 bytes of the runs parse), then the
// bytes (the non-final stream).  form: 0 stored, 1 fixed, 2 dynamic over the runs parse; 5 fixed, 6 dynamic over the window parse.
// Prints one line per mismatch and a summary line; the exit status is 0 unless a file cannot be read or written.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../spatiotemporal_variable_separation_amd/csrc/vs_deflate_window_core.h"
#include "../../spatiotemporal_variable_separation_amd/csrc/vs_inflate_core.h"

struct HostSink {
    uint8_t* out;
    int64_t pos;
    void lit(uint8_t v) { out[pos++] = v; }
    void copy(int dist, int len) {
        for (int i = 0; i < len; ++i, ++pos) out[pos] = out[pos - dist];
    }
    void stored(const uint8_t* src, int len) {
        memcpy(out + pos, src, (size_t)len);
        pos += len;
    }
    uint32_t adler() const {
        uint32_t a = 1, b = 0;
        for (int64_t i = 0; i < pos; ++i) {
            a = (a + out[i]) % 65521u;
            b = (b + a) % 65521u;
        }
        return (b << 16) | a;
    }
};

static int read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static int write_exact(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    const int chunk = atoi(argv[3]);
    if (!f || !g || chunk < 1 || chunk > VSD_MAX_CHUNK) return 2;
    int64_t records = 0;
    if (!read_exact(f, &records, 8) || !write_exact(g, &records, 8)) return 2;
    VsdWork* wr = (VsdWork*)malloc(sizeof(VsdWork));
    VsdWork* ww = (VsdWork*)malloc(sizeof(VsdWork));
    VsdWork* wref = (VsdWork*)malloc(sizeof(VsdWork));
    VswWork* ws = (VswWork*)malloc(sizeof(VswWork));
    VsiTables* tables = (VsiTables*)malloc(sizeof(VsiTables));
    long chunks_total = 0, mismatches = 0, forms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    {                                                                  // an empty chunk is the marker alone
        uint8_t* x = (uint8_t*)malloc(1);
        uint32_t* pk = (uint32_t*)malloc(4);
        uint32_t* img = (uint32_t*)malloc((size_t)vsd_image_words(0) * 4);
        const uint8_t marker[5] = {0, 0, 0, 0xFF, 0xFF};
        if (vsw_deflate_chunk(x, 0, 0, wr, ww, ws, pk, img, 0, 1) != 5 || memcmp(img, marker, 5) != 0 || ws->form != VSW_FORM_RUNS) {
            ++mismatches;
            printf("an empty chunk is not the five bytes of the marker\n");
        }
        free(x);
        free(pk);
        free(img);
    }
    for (int64_t r = 0; r < records; ++r) {
        int64_t history = 0, n = 0;
        if (!read_exact(f, &history, 8) || !read_exact(f, &n, 8) || n < 0 || history < 0 || history > VSW_MAX_HISTORY) return 2;
        uint8_t* all = (uint8_t*)malloc((size_t)(history + n) + 1);
        if (!all || !read_exact(f, all, (size_t)(history + n))) return 2;
        uint8_t* data = all + history;
        const int64_t n_chunks = (n + chunk - 1) / chunk;
        const int64_t cap = 2 + n + n_chunks * VSD_SLOT_EXTRA + 2 + 4;
        uint8_t* stream = (uint8_t*)malloc((size_t)cap);               // 78 01, the chunks, 03 00, Adler-32
        int32_t* meta = (int32_t*)malloc(n_chunks ? (size_t)n_chunks * 12 : 1);
        int64_t at = 2;
        stream[0] = 0x78;
        stream[1] = 0x01;
        for (int64_t c = 0; c < n_chunks; ++c) {
            const int len = (int)(n - c * chunk < chunk ? n - c * chunk : chunk);
            const int64_t before = history + c * chunk;
            const int hist = (int)(before < VSW_MAX_HISTORY ? before : VSW_MAX_HISTORY);
            uint8_t* y = (uint8_t*)malloc((size_t)(hist + len));       // exactly the history and the chunk
            uint32_t* pk = (uint32_t*)malloc((size_t)len * 4);
            uint32_t* img = (uint32_t*)malloc((size_t)vsd_image_words(len) * 4);
            uint32_t* ref = (uint32_t*)malloc((size_t)vsd_image_words(len) * 4);
            memcpy(y, data + c * chunk - hist, (size_t)(hist + len));
            memset(wr, 0xA5, sizeof(VsdWork));                         // nothing may depend on what a previous chunk left
            memset(ww, 0xA5, sizeof(VsdWork));
            memset(ws, 0xA5, sizeof(VswWork));
            memset(pk, 0xA5, (size_t)len * 4);
            memset(img, 0xA5, (size_t)vsd_image_words(len) * 4);
            const int size = vsw_deflate_chunk(y + hist, hist, len, wr, ww, ws, pk, img, 0, 1);
            const int runs = vsd_deflate_chunk(y + hist, len, wref, ref, 0, 1);
            const int form = ws->form;
            bool bad = size < 5 || size > len + VSD_SLOT_EXTRA || size > runs || (form != VSW_FORM_RUNS && form != VSD_FORM_FIXED && form != VSD_FORM_DYNAMIC);
            if (!bad && form == VSW_FORM_RUNS)
                bad = size != runs || memcmp(img, ref, (size_t)size) != 0 || ws->bits[1] < ws->bits[0] || ws->bits[2] < ws->bits[0];
            if (!bad && form != VSW_FORM_RUNS)
                bad = ws->bits[form] >= ws->bits[0] || ws->bits[3 - form] < ws->bits[form] || ws->bits[0] != wref->bits[wref->form];
            if (bad) {
                ++mismatches;
                printf("record %lld chunk %lld: %d bytes from %d (runs %d), form %d, bits %lld %lld %lld\n", (long long)r, (long long)c, size, len, runs,
                       form, (long long)ws->bits[0], (long long)ws->bits[1], (long long)ws->bits[2]);
                if (size < 0 || size > len + VSD_SLOT_EXTRA) return 3;
            }
            const int code = form == VSW_FORM_RUNS ? wr->form : 4 + form;
            ++forms[code & 7];
            memcpy(stream + at, img, (size_t)size);
            at += size;
            meta[3 * c] = code;
            meta[3 * c + 1] = size;
            meta[3 * c + 2] = runs;
            free(y);
            free(pk);
            free(img);
            free(ref);
        }
        chunks_total += n_chunks;
        const int64_t body = at - 2;
        if (history == 0) {
            stream[at++] = 0x03;
            stream[at++] = 0x00;
            HostSink ref = {data, n};
            const uint32_t adler = ref.adler();
            for (int k = 0; k < 4; ++k) stream[at++] = (uint8_t)(adler >> (24 - 8 * k));
            uint8_t* out = (uint8_t*)malloc(n ? (size_t)n : 1);
            HostSink sink = {out, 0};
            int64_t produced = -1;
            const int status = vsi_inflate_zlib(stream, at, n, tables, sink, &produced, 0, 1);
            if (status != 0 || produced != n || memcmp(out, data, (size_t)n) != 0) {
                ++mismatches;
                printf("record %lld: %lld bytes do not come back (status %d, produced %lld)\n", (long long)r, (long long)n, status, (long long)produced);
            }
            free(out);
        }
        if (!write_exact(g, &body, 8) || !write_exact(g, &n_chunks, 8) || !write_exact(g, meta, (size_t)n_chunks * 12) ||
            !write_exact(g, stream + 2, (size_t)body))
            return 2;
        free(meta);
        free(stream);
        free(all);
    }
    free(tables);
    free(ws);
    free(wref);
    free(ww);
    free(wr);
    fclose(f);
    if (fclose(g) != 0) return 2;
    printf("forms stored %ld fixed %ld dynamic %ld window-fixed %ld window-dynamic %ld\n", forms[0], forms[1], forms[2], forms[5], forms[6]);
    printf("records %lld chunks %ld mismatches %ld\n", (long long)records, chunks_total, mismatches);
    return 0;
}

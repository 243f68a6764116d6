// Host check of csrc/vs_deflate_core.h: the logic of vs_deflate_chunks and vs_crc32, compiled for the CPU (with sanitizers where they
// link) and run on a corpus file that tests/test_deflate_cpu.py writes.  Every chunk is compressed from an exactly-sized heap copy of its
// bytes into an exactly-sized heap image, so that a read or a write outside either is a sanitizer report.  Checked here: the slot bound,
// that the chosen block form is the smallest of the three by its own count, and that the chunks + a final block, framed as a zlib stream,
// inflate to the input through csrc/vs_inflate_core.h.  The emitted bytes go to an output file, where the test hands them to zlib and
// the GPU test compares them with the kernel's.
//
//   deflate_host_check CORPUS OUT CHUNK_BYTES
// CORPUS (little-endian): int64 records; per record int64 n and n bytes.
// OUT: int64 records; per record int64 bytes, int64 chunks, uint32 crc(init 0), uint32 crc(init 0xDEADBEEF), per chunk (int32 form, int32
// bytes), then the bytes (the non-final stream).  The CRCs are computed piecewise, CHUNK_BYTES per piece and 64 sub-pieces per piece.
// Prints one line per mismatch and a summary line; the exit status is 0 unless a file cannot be read or written.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../spatiotemporal_variable_separation_amd/csrc/vs_deflate_core.h"
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

static uint32_t piecewise_crc(const uint32_t* table, const uint8_t* data, int64_t n, int64_t piece, uint32_t init) {
    if (n == 0) return init;
    uint32_t acc = 0;
    for (int64_t lo = 0; lo < n; lo += piece) {
        const int64_t hi = lo + piece < n ? lo + piece : n;
        uint8_t* copy = (uint8_t*)malloc((size_t)(hi - lo));           // exactly the piece: nothing outside it may be read
        memcpy(copy, data + lo, (size_t)(hi - lo));
        for (int lane = 0; lane < 64; ++lane) acc ^= vsd_crc_partial(table, copy, n, lo, hi, init, lane, 64);
        free(copy);
    }
    return ~acc;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    const int chunk = atoi(argv[3]);
    if (!f || !g || chunk < 1 || chunk > VSD_MAX_CHUNK) return 2;
    int64_t records = 0;
    if (!read_exact(f, &records, 8) || !write_exact(g, &records, 8)) return 2;
    VsdWork* work = (VsdWork*)malloc(sizeof(VsdWork));
    VsiTables* tables = (VsiTables*)malloc(sizeof(VsiTables));
    uint32_t table[256];
    for (uint32_t b = 0; b < 256; ++b) table[b] = vsd_crc_table_entry(b);
    long chunks_total = 0, mismatches = 0, forms[4] = {0, 0, 0, 0};
    {                                                                  // an empty chunk is the marker alone
        uint8_t* x = (uint8_t*)malloc(1);
        uint32_t* img = (uint32_t*)malloc((size_t)vsd_image_words(0) * 4);
        const uint8_t marker[5] = {0, 0, 0, 0xFF, 0xFF};
        if (vsd_deflate_chunk(x, 0, work, img, 0, 1) != 5 || memcmp(img, marker, 5) != 0 || work->form != VSD_FORM_EMPTY) {
            ++mismatches;
            printf("an empty chunk is not the five bytes of the marker\n");
        }
        free(x);
        free(img);
    }
    for (int64_t r = 0; r < records; ++r) {
        int64_t n = 0;
        if (!read_exact(f, &n, 8) || n < 0) return 2;
        uint8_t* data = (uint8_t*)malloc(n ? (size_t)n : 1);
        if (!data || !read_exact(f, data, (size_t)n)) return 2;
        const int64_t n_chunks = (n + chunk - 1) / chunk;
        const int64_t cap = 2 + n + n_chunks * VSD_SLOT_EXTRA + 2 + 4;
        uint8_t* stream = (uint8_t*)malloc((size_t)cap);               // 78 01, the chunks, 03 00, Adler-32
        int32_t* meta = (int32_t*)malloc(n_chunks ? (size_t)n_chunks * 8 : 1);
        int64_t at = 2;
        stream[0] = 0x78;
        stream[1] = 0x01;
        for (int64_t c = 0; c < n_chunks; ++c) {
            const int len = (int)(n - c * chunk < chunk ? n - c * chunk : chunk);
            uint8_t* x = (uint8_t*)malloc((size_t)len);
            uint32_t* img = (uint32_t*)malloc((size_t)vsd_image_words(len) * 4);
            memcpy(x, data + c * chunk, (size_t)len);
            memset(work, 0xA5, sizeof(VsdWork));                       // nothing may depend on what a previous chunk left
            memset(img, 0xA5, (size_t)vsd_image_words(len) * 4);
            const int size = vsd_deflate_chunk(x, len, work, img, 0, 1);
            const int form = work->form;
            bool bad = size < 5 || size > len + VSD_SLOT_EXTRA || form < 0 || form > 2;
            if (!bad)
                for (int k = 0; k < 3; ++k) bad = bad || work->bits[k] < work->bits[form];
            if (bad) {
                ++mismatches;
                printf("record %lld chunk %lld: %d bytes from %d, form %d, bits %lld %lld %lld\n", (long long)r, (long long)c, size, len, form,
                       (long long)work->bits[0], (long long)work->bits[1], (long long)work->bits[2]);
                if (size < 0 || size > len + VSD_SLOT_EXTRA) return 3;
            }
            ++forms[form & 3];
            memcpy(stream + at, img, (size_t)size);
            at += size;
            meta[2 * c] = form;
            meta[2 * c + 1] = size;
            free(x);
            free(img);
        }
        chunks_total += n_chunks;
        const int64_t body = at - 2;
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
        const uint32_t crc[2] = {piecewise_crc(table, data, n, chunk, 0u), piecewise_crc(table, data, n, chunk, 0xDEADBEEFu)};
        if (!write_exact(g, &body, 8) || !write_exact(g, &n_chunks, 8) || !write_exact(g, crc, 8) || !write_exact(g, meta, (size_t)n_chunks * 8) ||
            !write_exact(g, stream + 2, (size_t)body))
            return 2;
        free(out);
        free(meta);
        free(stream);
        free(data);
    }
    free(tables);
    free(work);
    fclose(f);
    if (fclose(g) != 0) return 2;
    printf("forms stored %ld fixed %ld dynamic %ld\n", forms[0], forms[1], forms[2]);
    printf("records %lld chunks %ld mismatches %ld\n", (long long)records, chunks_total, mismatches);
    return 0;
}

// Host check of csrc/vs_inflate_core.h: the stream logic of vs_inflate_zlib, compiled for the CPU (with sanitizers where they link) and
// run on a corpus file that tests/test_png_decode_cpu.py writes.  Every record is decoded with exactly-sized heap buffers for the input
// and the output, so that a read or a write outside either is a sanitizer report, and compared with what zlib said about the stream.
//
// Corpus (little-endian): int64 records; per record int64 in_len, int64 out_len, int64 accepted, in_len bytes of stream and, when
// accepted, out_len bytes zlib produced.  A stream zlib refused must give a non-zero status with out_len as its output limit.
// Prints one line per mismatch and a summary line; the exit status is 0 unless the corpus cannot be read.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t records = 0;
    if (!read_exact(f, &records, 8)) return 2;
    VsiTables* tables = (VsiTables*)malloc(sizeof(VsiTables));
    long accepted = 0, refused = 0, mismatches = 0;
    for (int64_t r = 0; r < records; ++r) {
        int64_t head[3];
        if (!read_exact(f, head, sizeof(head))) return 2;
        const int64_t in_len = head[0], out_len = head[1], ok = head[2];
        uint8_t* in = (uint8_t*)malloc(in_len ? (size_t)in_len : 1);
        uint8_t* want = (uint8_t*)malloc(out_len ? (size_t)out_len : 1);
        uint8_t* out = (uint8_t*)malloc(out_len ? (size_t)out_len : 1);
        if (!in || !want || !out || !read_exact(f, in, (size_t)in_len) || (ok && !read_exact(f, want, (size_t)out_len))) return 2;
        memset(tables, 0xA5, sizeof(VsiTables));           // nothing may depend on what a previous stream left
        HostSink sink = {out, 0};
        int64_t produced = -1;
        const int status = vsi_inflate_zlib(in, in_len, out_len, tables, sink, &produced, 0, 1);
        if (ok) {
            ++accepted;
            if (status != 0 || produced != out_len || memcmp(out, want, (size_t)out_len) != 0) {
                ++mismatches;
                printf("record %lld: zlib accepts (%lld bytes), status %d, produced %lld\n", (long long)r, (long long)out_len, status, (long long)produced);
            }
        } else {
            ++refused;
            if (status == 0 || produced < 0 || produced > out_len) {
                ++mismatches;
                printf("record %lld: zlib refuses, status %d, produced %lld\n", (long long)r, status, (long long)produced);
            }
        }
        free(in);
        free(want);
        free(out);
    }
    free(tables);
    fclose(f);
    printf("records %lld accepted %ld refused %ld mismatches %ld\n", (long long)records, accepted, refused, mismatches);
    return 0;
}

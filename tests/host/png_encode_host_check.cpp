// Host check of csrc/vs_png_encode_core.h: the logic of vs_png_filter, vs_deflate_streams and vs_png_assemble, compiled for the CPU (with
// sanitizers where they link) and run on a case file that tests/test_png_encode_cpu.py and tests/test_png_encode_gpu.py write.  Every image
// is filtered from an exactly-sized heap copy of its own pixels into exactly S bytes, every chunk is compressed from an exactly-sized
// copy of its history + its bytes (the history taken from the image's own stream only), and every file is assembled into exactly the
// worst-case stride, so that a read or a write outside any of them -- the previous image's last row, a neighbouring stream -- is a
// sanitizer report.
//
//   png_encode_host_check CASES OUT
// CASES (little-endian): int64 records; per record int64 n, H, W, C, mode (0..4, 5 adaptive), chunk_bytes, match (0 runs, 1 window) and
// n * H * W * C bytes of pixels.
// OUT: int64 records; per record int64 n, int64 S, the n * S filtered bytes, then per image int64 file bytes and the file.
// Prints a summary line; the exit status is 0 unless a file cannot be read or written or a record is malformed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../spatiotemporal_variable_separation_amd/csrc/vs_png_encode_core.h"

static int read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static int write_exact(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    int64_t records = 0;
    if (!read_exact(f, &records, 8) || !write_exact(g, &records, 8)) return 2;
    VsdWork* wr = (VsdWork*)malloc(sizeof(VsdWork));
    VsdWork* ww = (VsdWork*)malloc(sizeof(VsdWork));
    VswWork* ws = (VswWork*)malloc(sizeof(VswWork));
    uint32_t table[256];
    for (uint32_t b = 0; b < 256; ++b) table[b] = vsd_crc_table_entry(b);
    long images = 0, chunks_total = 0, refused = 0;
    for (int64_t r = 0; r < records; ++r) {
        int64_t h[7];
        if (!read_exact(f, h, sizeof h)) return 2;
        const int64_t n = h[0], H = h[1], W = h[2], C = h[3], mode = h[4], chunk = h[5], match = h[6];
        if (n < 1 || H < 1 || W < 1 || C < 1 || C > 4 || mode < 0 || mode > VPE_MODE_ADAPTIVE || chunk < 1 || chunk > VSD_MAX_CHUNK || match < 0 ||
            match > 1 || W * C > 65535)
            return 2;
        const int row_bytes = (int)(W * C);
        const int64_t image_bytes = H * row_bytes, S = H * (row_bytes + 1), K = vpe_chunks_per_stream(S, (int)chunk);
        const int64_t slot_stride = chunk + VSD_SLOT_EXTRA, file_stride = vpe_file_bound(S, K);
        const VpeLead lead = vpe_lead((int)W, (int)H, (int)C);
        uint8_t** raws = (uint8_t**)malloc((size_t)n * sizeof(uint8_t*));
        uint8_t** files = (uint8_t**)malloc((size_t)n * sizeof(uint8_t*));
        int64_t* file_bytes = (int64_t*)malloc((size_t)n * 8);
        for (int64_t i = 0; i < n; ++i) {
            uint8_t* pixels = (uint8_t*)malloc((size_t)image_bytes);       // exactly this image: the row above row 0 is not the previous image's
            uint8_t* raw = (uint8_t*)malloc((size_t)S);
            if (!pixels || !raw || !read_exact(f, pixels, (size_t)image_bytes)) return 2;
            for (int64_t y = 0; y < H; ++y)
                vpe_filter_row(pixels + y * row_bytes, y > 0 ? pixels + (y - 1) * row_bytes : nullptr, row_bytes, (int)C, (int)mode,
                               raw + y * (row_bytes + 1));
            uint8_t* slots = (uint8_t*)malloc((size_t)(K * slot_stride));
            int64_t* sizes = (int64_t*)malloc((size_t)K * 8);
            for (int64_t k = 0; k < K; ++k) {
                int64_t lo;
                int len, hist;
                vpe_chunk(S, (int)chunk, k, &lo, &len, &hist);
                if (match == 0) hist = 0;
                uint8_t* y = (uint8_t*)malloc((size_t)(hist + len));       // exactly the history and the chunk
                uint32_t* pk = (uint32_t*)malloc((size_t)len * 4);
                uint32_t* img = (uint32_t*)malloc((size_t)vsd_image_words(len) * 4);
                memcpy(y, raw + lo - hist, (size_t)(hist + len));
                memset(wr, 0xA5, sizeof(VsdWork));                         // nothing may depend on what a previous chunk left
                memset(ww, 0xA5, sizeof(VsdWork));
                memset(ws, 0xA5, sizeof(VswWork));
                memset(pk, 0xA5, (size_t)len * 4);
                memset(img, 0xA5, (size_t)vsd_image_words(len) * 4);
                const int size = match == 0 ? vsd_deflate_chunk(y, len, wr, img, 0, 1) : vsw_deflate_chunk(y + hist, hist, len, wr, ww, ws, pk, img, 0, 1);
                if (size < 5 || size > len + VSD_SLOT_EXTRA) return 3;
                memcpy(slots + k * slot_stride, img, (size_t)size);
                sizes[k] = size;
                free(y);
                free(pk);
                free(img);
            }
            chunks_total += (long)K;
            uint8_t* file = (uint8_t*)malloc((size_t)file_stride);
            memset(file, 0xA5, (size_t)file_stride);
            file_bytes[i] = vpe_assemble(file, file_stride, lead, slots, slot_stride, sizes, K, raw, S, table, 0, 1);
            {                                                              // a size outside its slot is refused, and nothing is written
                uint8_t* other = (uint8_t*)malloc((size_t)file_stride);
                memset(other, 0xA5, (size_t)file_stride);
                const int64_t kept = sizes[K - 1];
                int bad = 0;
                sizes[K - 1] = slot_stride + 1;
                bad |= vpe_assemble(other, file_stride, lead, slots, slot_stride, sizes, K, raw, S, table, 0, 1) != -1;
                sizes[K - 1] = -1;
                bad |= vpe_assemble(other, file_stride, lead, slots, slot_stride, sizes, K, raw, S, table, 0, 1) != -1;
                sizes[K - 1] = kept;
                for (int64_t b = 0; b < file_stride; ++b) bad |= other[b] != 0xA5;
                if (bad) printf("record %lld image %lld: a size outside its slot was not refused cleanly\n", (long long)r, (long long)i);
                else ++refused;
                free(other);
            }
            raws[i] = raw;
            files[i] = file;
            ++images;
            free(sizes);
            free(slots);
            free(pixels);
        }
        if (!write_exact(g, &n, 8) || !write_exact(g, &S, 8)) return 2;
        for (int64_t i = 0; i < n; ++i)
            if (!write_exact(g, raws[i], (size_t)S)) return 2;
        for (int64_t i = 0; i < n; ++i) {
            if (file_bytes[i] < 0 || file_bytes[i] > file_stride) return 3;
            if (!write_exact(g, &file_bytes[i], 8) || !write_exact(g, files[i], (size_t)file_bytes[i])) return 2;
            free(raws[i]);
            free(files[i]);
        }
        free(file_bytes);
        free(files);
        free(raws);
    }
    free(ws);
    free(ww);
    free(wr);
    fclose(f);
    if (fclose(g) != 0) return 2;
    printf("records %lld images %ld chunks %ld refusals %ld\n", (long long)records, images, chunks_total, refused);
    return 0;
}

// vs_png_encode_core.h -- the logic of the PNG encoder (csrc/vs_png_encode.hip) as plain __host__ __device__ functions, on top of the two
// DEFLATE cores: the forward row filters with the adaptive choice, the cut of a stream into chunks that see only their own stream, and the
// framing of one file (signature, IHDR, one IDAT around the chunks with its Adler-32 and CRC-32, IEND).  The header compiles with a host
// compiler alone (tests/host/png_encode_host_check.cpp): one logic, two builds, the kernels' bytes are the host's bytes.
//
// Filters (PNG 1.2, section 6; bpp = C).  Every residual depends on SOURCE pixels only -- x, a (left), b (above), c (above left) -- so rows
// and bytes are independent; the row above row 0 of EVERY image is zeros, and so is the pixel left of column 0.  The adaptive choice of a
// row is the type with the least sum of |residual|, each residual read as a signed byte (0x80 counts 128); a tie goes to the lowest type.
//
// Streams.  Stream s of stream_bytes bytes is cut into K = ceil(stream_bytes / chunk_bytes) chunks; chunk k sees min(32768, k *
// chunk_bytes) bytes of history, which are the stream's own bytes: vpe_chunk says where a chunk lies.  The chunk itself is
// vsd_deflate_chunk or vsw_deflate_chunk, unchanged.
//
// Files.  vpe_assemble writes one file: `lane` of `nlanes` (host: 0 of 1; device: a workgroup's threads) stripe every copy and every sum.
// Besides VSD_SYNC two primitives with host defaults: VPE_SUM and VPE_XOR (the sum / the XOR of a 32-bit value over the lanes, the same
// result in every lane).  The CRC-32 of the IDAT chunk is computed from the bytes of the file just written, after a VSD_SYNC.
//
// Bounds, on ANY input: vpe_assemble reads K sizes and refuses (-1, nothing written) unless every size is inside 0 .. slot_stride and the
// whole file fits file_stride, so a copy never leaves a slot or the file; the Adler-32 reads S bytes of raw in pieces of VPE_ADLER_PIECE,
// whose per-lane sums stay below 2^32 (255 * 4096 * 4097 / 2 < 2^32 for one lane that takes a whole piece).
#pragma once
#include "vs_deflate_window_core.h"

#ifndef VPE_SUM
#define VPE_SUM(v) (v)
#define VPE_XOR(v) (v)
#endif

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VPE_HH __host__ __device__ inline           /* also for the host side of a device build: the entry points call these */
#else
#define VPE_HH inline
#endif

#define VPE_MODE_ADAPTIVE 5
#define VPE_LEAD_BYTES 33                           /* signature + IHDR chunk: the same for every image of a batch */
#define VPE_FIXED_BYTES 65                          /* 57 + 8: everything of a file but the chunks */
#define VPE_ADLER_PIECE 4096
#define VPE_ADLER_MOD 65521u

struct VpeLead {
    uint8_t b[VPE_LEAD_BYTES + 3];                  // (a multiple of 4: passed to the kernel by value)
};

// ---- filters -----------------------------------------------------------------------------------------------------------------------
VPE_HH int vpe_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// the filtered byte of type f (0..4) for x with a = left, b = above, c = above left
VPE_HH uint32_t vpe_residual(int f, int x, int a, int b, int c) {
    const int pred = f == 1 ? a : f == 2 ? b : f == 3 ? ((a + b) >> 1) : f == 4 ? vpe_paeth(a, b, c) : 0;
    return (uint32_t)(x - pred) & 255u;
}
// |r| of a residual read as a signed byte
VPE_HH uint32_t vpe_cost(uint32_t r) { return r < 128u ? r : 256u - r; }
// the five costs of one byte, added to sums[0 .. 5)
VPE_HH void vpe_add_costs(uint32_t* sums, int x, int a, int b, int c) {
    sums[0] += vpe_cost((uint32_t)x);
    sums[1] += vpe_cost((uint32_t)(x - a) & 255u);
    sums[2] += vpe_cost((uint32_t)(x - b) & 255u);
    sums[3] += vpe_cost((uint32_t)(x - ((a + b) >> 1)) & 255u);
    sums[4] += vpe_cost((uint32_t)(x - vpe_paeth(a, b, c)) & 255u);
}
// the type with the least sum; a tie goes to the lowest type
VPE_HH int vpe_choose(const uint32_t* sums) {
    int f = 0;
    for (int t = 1; t < 5; ++t)
        if (sums[t] < sums[f]) f = t;
    return f;
}
// One row on one lane, byte by byte (the host's form; the kernel stripes the same functions over a wave, four bytes per lane):
// cur [row_bytes] = W * C bytes, up: the row above or NULL for zeros; out [1 + row_bytes].  Returns the type written.
VPE_HH int vpe_filter_row(const uint8_t* cur, const uint8_t* up, int row_bytes, int C, int mode, uint8_t* out) {
    int f = mode;
    if (mode == VPE_MODE_ADAPTIVE) {
        uint32_t sums[5] = {0u, 0u, 0u, 0u, 0u};
        for (int j = 0; j < row_bytes; ++j)
            vpe_add_costs(sums, cur[j], j >= C ? cur[j - C] : 0, up ? up[j] : 0, (up && j >= C) ? up[j - C] : 0);
        f = vpe_choose(sums);
    }
    out[0] = (uint8_t)f;
    for (int j = 0; j < row_bytes; ++j)
        out[1 + j] = (uint8_t)vpe_residual(f, cur[j], j >= C ? cur[j - C] : 0, up ? up[j] : 0, (up && j >= C) ? up[j - C] : 0);
    return f;
}

// ---- streams -----------------------------------------------------------------------------------------------------------------------
VPE_HH int64_t vpe_chunks_per_stream(int64_t stream_bytes, int chunk_bytes) { return (stream_bytes + chunk_bytes - 1) / chunk_bytes; }
// chunk k of a stream: its offset inside the stream, its length (1 .. chunk_bytes) and the history before it -- the stream's own bytes
VPE_HH void vpe_chunk(int64_t stream_bytes, int chunk_bytes, int64_t k, int64_t* lo, int* n, int* hist) {
    *lo = k * (int64_t)chunk_bytes;
    *n = (int)(stream_bytes - *lo < chunk_bytes ? stream_bytes - *lo : chunk_bytes);
    *hist = (int)(*lo < VSW_MAX_HISTORY ? *lo : VSW_MAX_HISTORY);
}

// ---- framing -----------------------------------------------------------------------------------------------------------------------
VPE_HH int vpe_colour_type(int C) { return C == 1 ? 0 : C == 2 ? 4 : C == 3 ? 2 : 6; }
VPE_HH int64_t vpe_file_bound(int64_t S, int64_t K) { return VPE_FIXED_BYTES + S + (int64_t)VSD_SLOT_EXTRA * K; }
VPE_HH uint32_t vpe_crc_byte(uint32_t c, uint8_t v) {   // bit by bit: the 17 bytes of an IHDR need no table
    c ^= v;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    return c;
}
VPE_HH void vpe_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}
// the 33 bytes every file of W x H pixels of C channels starts with
VPE_HH VpeLead vpe_lead(int W, int H, int C) {
    const uint8_t magic[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    VpeLead l;
    for (int i = 0; i < 8; ++i) l.b[i] = magic[i];
    vpe_be32(l.b + 8, 13u);
    l.b[12] = 'I'; l.b[13] = 'H'; l.b[14] = 'D'; l.b[15] = 'R';
    vpe_be32(l.b + 16, (uint32_t)W);
    vpe_be32(l.b + 20, (uint32_t)H);
    l.b[24] = 8; l.b[25] = (uint8_t)vpe_colour_type(C); l.b[26] = 0; l.b[27] = 0; l.b[28] = 0;
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 12; i < 29; ++i) c = vpe_crc_byte(c, l.b[i]);
    vpe_be32(l.b + 29, ~c);
    l.b[33] = l.b[34] = l.b[35] = 0;
    return l;
}

// dst[0 .. n) = src[0 .. n): the destination in words where it is aligned (the source by bytes: it is in cache), bytes at both ends
VSD_HD void vpe_copy(uint8_t* dst, const uint8_t* src, int64_t n, int lane, int nlanes) {
    int64_t head = (int64_t)((4 - ((uintptr_t)dst & 3)) & 3);
    if (head > n) head = n;
    for (int64_t i = lane; i < head; i += nlanes) dst[i] = src[i];
    const int64_t words = (n - head) >> 2;
    for (int64_t w = lane; w < words; w += nlanes) {
        const uint8_t* p = src + head + 4 * w;
        *reinterpret_cast<uint32_t*>(__builtin_assume_aligned(dst + head + 4 * w, 4)) =
            (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    }
    for (int64_t i = head + 4 * words + lane; i < n; i += nlanes) dst[i] = src[i];
}

// Adler-32 of raw[0 .. S) as vs_png.hip's sink computes it: per piece, every lane sums its bytes and (len - i) * byte, one reduction
VSD_HD uint32_t vpe_adler(const uint8_t* raw, int64_t S, int lane, int nlanes) {
    uint32_t a = 1u, b = 0u;
    for (int64_t at = 0; at < S; at += VPE_ADLER_PIECE) {
        const int len = (int)(S - at < VPE_ADLER_PIECE ? S - at : VPE_ADLER_PIECE);
        const uint8_t* p = raw + at;
        uint32_t s1 = 0, s2 = 0;
        if (((uintptr_t)p & 3) == 0 && len == VPE_ADLER_PIECE) {
            for (int i = 4 * lane; i < VPE_ADLER_PIECE; i += 4 * nlanes) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(__builtin_assume_aligned(p + i, 4));
                for (int k = 0; k < 4; ++k) {
                    const uint32_t v = (w >> (8 * k)) & 255u;
                    s1 += v;
                    s2 += (uint32_t)(VPE_ADLER_PIECE - i - k) * v;
                }
            }
        } else {
            for (int i = lane; i < len; i += nlanes) {
                const uint32_t v = p[i];
                s1 += v;
                s2 += (uint32_t)(len - i) * v;
            }
        }
        s1 = VPE_SUM(s1 % VPE_ADLER_MOD);               // at most nlanes * 65520: below 2^32 for any workgroup
        s2 = VPE_SUM(s2 % VPE_ADLER_MOD);
        b = (uint32_t)(((uint64_t)b + (uint64_t)len * a + s2) % VPE_ADLER_MOD);   // after len bytes: b' = b + len * a + sum (len - i) * byte
        a = (a + s1) % VPE_ADLER_MOD;
    }
    return (b << 16) | a;
}

// One file: lead, IDAT (78 9C, the K slots back to back, 03 00, the Adler-32 of raw[0 .. S)), IEND, into file[0 .. file_stride).
// table: the 256 entries of vsd_crc_table_entry.  Returns the file's bytes = VPE_FIXED_BYTES + the K sizes, or -1 (and nothing written)
// when a size is outside 0 .. slot_stride or the file would not fit; the same value in every lane.  `file` is read back for the CRC, so it
// is no __restrict__ pointer: VSD_SYNC orders the lanes' own writes to it before their reads of it.
VSD_HD int64_t vpe_assemble(uint8_t* file, int64_t file_stride, const VpeLead& lead, const uint8_t* slots, int64_t slot_stride, const int64_t* sizes,
                            int64_t K, const uint8_t* raw, int64_t S, const uint32_t* table, int lane, int nlanes) {
    int64_t total = 0;
    for (int64_t k = 0; k < K; ++k) {                   // every lane reads every size: the verdict is uniform without a reduction
        const int64_t size = sizes[k];
        if (size < 0 || size > slot_stride || size > file_stride) return -1;
        total += size;
        if (total > file_stride) return -1;
    }
    if (total > file_stride - VPE_FIXED_BYTES) return -1;
    const int64_t body = total + 8;                     // 78 9C ... 03 00 + Adler-32
    uint8_t* idat = file + VPE_LEAD_BYTES;              // length, "IDAT", body, CRC
    const uint8_t after[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    const uint8_t kind[6] = {'I', 'D', 'A', 'T', 0x78, 0x9C};
    for (int i = lane; i < VPE_LEAD_BYTES + 10; i += nlanes)
        file[i] = i < VPE_LEAD_BYTES ? lead.b[i] : i < VPE_LEAD_BYTES + 4 ? (uint8_t)((uint64_t)body >> (8 * (VPE_LEAD_BYTES + 3 - i))) : kind[i - VPE_LEAD_BYTES - 4];
    int64_t at = 10;                                    // inside idat
    for (int64_t k = 0; k < K; ++k) {
        vpe_copy(idat + at, slots + k * slot_stride, sizes[k], lane, nlanes);
        at += sizes[k];
    }
    const uint32_t adler = vpe_adler(raw, S, lane, nlanes);
    for (int i = lane; i < 6; i += nlanes) idat[at + i] = i == 0 ? 0x03 : i == 1 ? 0x00 : (uint8_t)(adler >> (8 * (5 - i)));
    at += 6;
    for (int i = lane; i < 12; i += nlanes) idat[at + 4 + i] = after[i];
    VSD_SYNC();                                         // the chunk's bytes are written: every lane may read them
    const int64_t n = 4 + body;                         // what the CRC covers: "IDAT" + body
    const uint32_t crc = ~VPE_XOR(vsd_crc_partial(table, idat + 4, n, 0, n, 0u, lane, nlanes));
    for (int i = lane; i < 4; i += nlanes) idat[at + i] = (uint8_t)(crc >> (8 * (3 - i)));
    return VPE_FIXED_BYTES + total;
}

// vs_png.hip -- PNG decoding on the device: vs_inflate_zlib (the IDAT streams of a batch, one wave per stream) and vs_png_unfilter (the
// filtered rows into pixels).  The compressed files of a batch are a few hundred times smaller than their pixels, and the renders are
// independent, so decoding them here replaces the host's decode stage AND the upload of the decoded pixels.
//
// vs_inflate_zlib.  The stream logic (bit reader, framing, tables, symbols, every check) is csrc/vs_inflate_core.h, which also runs on the
// CPU; this file adds where the bytes go.  ONE WORKGROUP OF ONE WAVE PER STREAM.  All 64 lanes run the decoder with the same values, so
// control flow is wave-uniform and a table entry or an input byte is one broadcast read.  Per workgroup, in LDS (about 39.5 KiB: four
// workgroups per CU):
//   * the two code tables of the current block (3.5 KiB);
//   * WINDOW, a ring of 36 KiB = the 32 KiB of history DEFLATE may reach back into + 4 KiB.  A literal is one byte store by lane 0; a match
//     is copied by all lanes, `ring[pos + i] = ring[pos - dist + i]` for dist >= 64 (64 bytes per turn, a turn reads only what earlier
//     turns wrote) and `ring[pos + i] = ring[pos - dist + i % dist]` below (reads only what was there before the match), which is correct
//     for overlapping copies.  LDS operations of a wave execute in program order, so a byte written by one lane is there for another
//     lane's later read; a wave-scope fence keeps the compiler from reordering across the phases.
//   * Whenever 4 KiB are complete, the wave writes them to the slot (coalesced dwords when the slot address allows, bytes otherwise) and adds
//     them to the Adler-32 (per-lane partial sums, one wave reduction per piece).  Global memory is only ever written, never read back.
// Writing 258 bytes at `pos` overwrites ring bytes at least 36 KiB - 258 back: older than any distance, and flushed long before.
//
// vs_png_unfilter.  ONE WORKGROUP PER IMAGE, ONE WAVE PER CHANNEL (bpp = C: the channels never meet).  A wave takes 64 rows at a time as a
// skewed wavefront: lane k works on row y0 + k and is one pixel behind lane k - 1, so at every step the byte above (and, one step older,
// above-left) is what the neighbouring lane produced in the previous step -- one lane shift, whatever the filter types of the two rows.
// The left byte is the lane's own previous result.  The last row of a band is kept in LDS for lane 0 of the next band.  Each lane
// predicts with all five filters and selects by its row's type: no divergence between rows of different types.
#include "vs_common.h"

#define VSI_SYNC() __syncthreads()
#include "vs_inflate_core.h"

namespace {

constexpr int INF_RING = 36 * 1024;           // history window + room to write ahead
constexpr int INF_PIECE = 4096;               // bytes per flush; INF_RING is a multiple, so a piece never wraps
constexpr int INF_STORED_PIECE = 2048;        // bytes of a stored block written between two flush checks
constexpr uint32_t ADLER_MOD = 65521u;

__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// The kernel's sink: the ring in LDS, flushed to the output slot piece by piece.  pos is the number of bytes produced, rp = pos % INF_RING.
struct RingSink {
    uint8_t* ring;
    uint8_t* out;                             // the slot
    int lane;
    int64_t pos, flushed;                     // flushed: a multiple of INF_PIECE
    int rp;
    uint32_t a, b;                            // Adler-32 of the flushed bytes
    bool dwords;                              // the slot is 4-byte aligned

    // bytes [flushed, flushed + len) of the output, len <= INF_PIECE, contiguous in the ring
    __device__ void flush(int len) {
        wave_fence();
        const int r0 = (int)(flushed % INF_RING);
        const uint8_t* src = ring + r0;
        uint8_t* dst = out + flushed;
        uint32_t s1 = 0, s2 = 0;              // sum of the bytes, and of (len - i) * byte: below 64 * 255 * 4096 < 2^32 per lane
        if (dwords && len == INF_PIECE) {
            for (int i = lane * 4; i < INF_PIECE; i += 256) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(src + i);
                *reinterpret_cast<uint32_t*>(dst + i) = w;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t v = (w >> (8 * k)) & 255u;
                    s1 += v;
                    s2 += (uint32_t)(INF_PIECE - i - k) * v;
                }
            }
        } else {
            for (int i = lane; i < len; i += 64) {
                const uint32_t v = src[i];
                dst[i] = (uint8_t)v;
                s1 += v;
                s2 += (uint32_t)(len - i) * v;
            }
        }
        s1 = wave_sum(s1 % ADLER_MOD);
        s2 = wave_sum(s2 % ADLER_MOD);
        // after len bytes: a' = a + s1, b' = b + len * a + sum (len - i) * byte
        b = (uint32_t)(((uint64_t)b + (uint64_t)len * a + s2) % ADLER_MOD);
        a = (a + s1) % ADLER_MOD;
        flushed += len;
    }
    __device__ void advance(int len) {
        pos += len;
        rp += len;
        if (rp >= INF_RING) rp -= INF_RING;
        if (pos - flushed >= INF_PIECE) flush(INF_PIECE);
    }
    __device__ void lit(uint8_t v) {
        if (lane == 0) ring[rp] = v;
        advance(1);
    }
    __device__ void copy(int dist, int len) {  // 1 <= dist <= min(pos, 32768), 3 <= len <= 258
        int sp = rp - dist;
        if (sp < 0) sp += INF_RING;
        wave_fence();
        if (dist >= 64) {
            for (int j = 0; j < len; j += 64) {
                const int i = j + lane;
                if (i < len) {
                    int s = sp + i, d = rp + i;
                    if (s >= INF_RING) s -= INF_RING;
                    if (d >= INF_RING) d -= INF_RING;
                    ring[d] = ring[s];
                }
                wave_fence();
            }
        } else {
            for (int j = 0; j < len; j += 64) {
                const int i = j + lane;
                if (i < len) {
                    int s = sp + (int)((unsigned)i % (unsigned)dist), d = rp + i;
                    if (s >= INF_RING) s -= INF_RING;
                    if (d >= INF_RING) d -= INF_RING;
                    ring[d] = ring[s];
                }
            }
        }
        advance(len);
    }
    __device__ void stored(const uint8_t* src, int len) {
        for (int done = 0; done < len; done += INF_STORED_PIECE) {        // at most 32 turns
            const int m = len - done < INF_STORED_PIECE ? len - done : INF_STORED_PIECE;
            for (int i = lane; i < m; i += 64) {
                int d = rp + i;
                if (d >= INF_RING) d -= INF_RING;
                ring[d] = src[done + i];
            }
            advance(m);
        }
    }
    __device__ uint32_t adler() {             // flushes what is left: at most INF_PIECE - 1 bytes
        if (pos > flushed) flush((int)(pos - flushed));
        return (b << 16) | a;
    }
};

struct InflateArgs {
    const uint8_t* packed;
    int64_t packed_bytes;
    const int64_t* offsets;
    const int64_t* out_len;
    uint8_t* out;
    int64_t out_stride;
    int32_t* status;
    int64_t* produced;
};

__global__ __launch_bounds__(64) void inflate_zlib_kernel(const InflateArgs a) {
    __shared__ VsiTables tables;
    __shared__ __attribute__((aligned(16))) uint8_t ring[INF_RING];
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t lo = a.offsets[s], hi = a.offsets[s + 1], want = a.out_len[s];
    int st;
    int64_t made = 0;
    if (lo < 0 || hi < lo || hi > a.packed_bytes) {
        st = VS_INFLATE_INPUT;
    } else if (want < 0 || want > a.out_stride) {
        st = VS_INFLATE_OUT_LONG;
    } else {
        RingSink sink;
        sink.ring = ring;
        sink.out = a.out + s * a.out_stride;
        sink.lane = lane;
        sink.pos = 0; sink.flushed = 0; sink.rp = 0;
        sink.a = 1u; sink.b = 0u;
        sink.dwords = ((uintptr_t)sink.out & 3) == 0;
        st = vsi_inflate_zlib(a.packed + lo, hi - lo, want, &tables, sink, &made, lane, 64);
        if (st != VS_INFLATE_OK && sink.pos > sink.flushed) sink.flush((int)(sink.pos - sink.flushed));   // what was produced before the failure
    }
    if (lane == 0) {
        a.status[s] = st;
        a.produced[s] = made;
    }
}

// ---- the row filters ----------------------------------------------------------------------------------------------------------------
constexpr int UF_STEPS = 4;                   // pixels per lane whose filtered bytes are loaded before the first is used

__global__ __launch_bounds__(256) void png_unfilter_kernel(const uint8_t* __restrict__ raw, int64_t raw_stride, int H, int W, int C,
                                                           uint8_t* __restrict__ pixels, int32_t* status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t above[];        // [C][W]: the last row of the previous band
    const int64_t img = blockIdx.x;
    if (status[img] != 0) return;             // failed in the inflate launch (or flagged by this image's first wave): nothing to decode
    const int k = threadIdx.x & 63, c = threadIdx.x >> 6;
    const int row_bytes = 1 + W * C;
    const uint8_t* src = raw + img * raw_stride;
    uint8_t* dst = pixels + img * (int64_t)H * W * C;
    uint8_t* up_row = above + c * W;
    for (int y0 = 0; y0 < H; y0 += 64) {      // bands of 64 rows
        const int y = y0 + k;
        const bool active = y < H;
        const uint8_t* in = src + (int64_t)(active ? y : 0) * row_bytes;
        uint8_t* o = dst + (int64_t)(active ? y : 0) * W * C + c;
        int ft = active ? in[0] : 0;
        if (ft > 4) {
            if (c == 0) status[img] = VS_PNG_BAD_FILTER;
            ft = 0;
        }
        in += 1 + c;
        const bool last = k == 63 || y == H - 1;                            // the row the next band continues from
        int cur = 0, left = 0, upleft = 0;
        for (int t0 = 0; t0 < W + 63; t0 += UF_STEPS) {                     // lane k is at pixel t - k in step t
            int f[UF_STEPS];
#pragma unroll
            for (int u = 0; u < UF_STEPS; ++u) {
                const int x = t0 + u - k;
                f[u] = (active && x >= 0 && x < W) ? in[x * C] : 0;
            }
#pragma unroll
            for (int u = 0; u < UF_STEPS; ++u) {
                const int x = t0 + u - k;
                const bool valid = active && x >= 0 && x < W;
                int up = __shfl_up(cur, 1, 64);                             // what lane k - 1 made in the previous step: pixel x of row y - 1
                if (k == 0) up = (y0 > 0 && valid) ? up_row[x] : 0;
                if (valid) {
                    if (x == 0) {
                        left = 0;
                        upleft = 0;
                    }
                    const int p = left + up - upleft;
                    const int pa = abs(p - left), pb = abs(p - up), pc = abs(p - upleft);
                    const int paeth = (pa <= pb && pa <= pc) ? left : (pb <= pc ? up : upleft);
                    const int pred = ft == 1 ? left : ft == 2 ? up : ft == 3 ? ((left + up) >> 1) : ft == 4 ? paeth : 0;
                    cur = (f[u] + pred) & 255;
                    o[(int64_t)x * C] = (uint8_t)cur;
                    if (last) up_row[x] = (uint8_t)cur;
                    left = cur;
                    upleft = up;
                }
            }
        }
    }
}

}  // namespace

extern "C" int vs_inflate_zlib(const uint8_t* packed, int64_t packed_bytes, const int64_t* offsets, int64_t n, const int64_t* out_len,
                               uint8_t* out, int64_t out_stride, int32_t* status, int64_t* produced, void* stream) {
    VS_CHECK_ARG(packed && offsets && out_len && out && status && produced, "vs_inflate_zlib: null pointer");
    VS_CHECK_ARG(n > 0 && packed_bytes >= 0 && out_stride > 0, "vs_inflate_zlib: sizes must be positive (n %lld, packed bytes %lld, out_stride %lld)",
                 (long long)n, (long long)packed_bytes, (long long)out_stride);
    VS_CHECK_ARG(n <= 2147483647ll, "vs_inflate_zlib: %lld streams exceed the grid limit", (long long)n);
    InflateArgs a;
    a.packed = packed; a.packed_bytes = packed_bytes; a.offsets = offsets; a.out_len = out_len;
    a.out = out; a.out_stride = out_stride; a.status = status; a.produced = produced;
    hipLaunchKernelGGL(inflate_zlib_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, a);
    VS_CHECK_LAUNCH("vs_inflate_zlib");
    return VS_OK;
}

extern "C" int vs_png_unfilter(const uint8_t* raw, int64_t raw_stride, int64_t n, int H, int W, int C, uint8_t* pixels, int32_t* status,
                               void* stream) {
    VS_CHECK_ARG(raw && pixels && status, "vs_png_unfilter: null pointer");
    VS_CHECK_ARG(n > 0 && H > 0 && W > 0, "vs_png_unfilter: sizes must be positive (n %lld, image %d x %d)", (long long)n, H, W);
    VS_CHECK_ARG(C >= 1 && C <= 4, "vs_png_unfilter: 1..4 channels (got %d)", C);
    VS_CHECK_ARG((int64_t)W * C <= 65536, "vs_png_unfilter: a row of %lld bytes exceeds the 65536 kept in LDS", (long long)W * C);
    VS_CHECK_ARG(raw_stride >= (int64_t)H * (1 + (int64_t)W * C), "vs_png_unfilter: raw_stride %lld is less than the %d rows of %lld bytes",
                 (long long)raw_stride, H, 1 + (long long)W * C);
    VS_CHECK_ARG(n <= 2147483647ll, "vs_png_unfilter: %lld images exceed the grid limit", (long long)n);
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)n), dim3(64 * C), (size_t)W * C, (hipStream_t)stream, raw, raw_stride, H, W, C, pixels,
                       status);
    VS_CHECK_LAUNCH("vs_png_unfilter");
    return VS_OK;
}

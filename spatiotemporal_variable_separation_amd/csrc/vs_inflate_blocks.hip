// vs_inflate_blocks.hip -- block-parallel DEFLATE decoding on the device, the reader of the .npz members that zlib (np.savez_compressed)
// writes: one unbroken raw RFC 1951 stream, no sync markers.  vs_inflate_block_scan (where dynamic blocks may start), vs_inflate_block_probe
// (one wave per candidate, window unknown), vs_inflate_block_windows (the true 32 KiB before every span of the chain) and
// vs_inflate_block_decode (one wave per span of the chain, window known, straight into the output).  The logic is
// csrc/vs_inflate_blocks_core.h, which also runs on the CPU; the host walks the chain over the small report table (ops.inflate_blocks).  No
// kernel waits on another workgroup: order comes from launch order and from the single workgroup of vs_inflate_block_windows.
//
// vs_inflate_block_scan.  A thread owns the 32 bit positions of 4 bytes and reads 16 bytes.  vsb_quick (17 header bits and the Kraft sum of
// the code-length code) leaves about one position in 500; a thread then validates its survivors one after the other with a bit reader of its
// own, the lanes of a wave side by side (vsb_block_start: the code-length code in two packed words, the lengths as counts per length, no
// array indexed at run time).  A wave appends its matches with one atomic; the list is unordered and the count goes on past the capacity.
//
// vs_inflate_block_scan_stored (opt-in, ops.inflate_block_scan(stored=True)).  The same split of the stream, one pass at memory rate: a
// thread tests its four byte boundaries for LEN / NLEN = ~LEN with LEN + 1 bytes behind them and counts the zero bits in front of each
// (vsb_stored_boundary, vsb_stored_count); a boundary appends up to eight adjacent bit positions.  Bit 0 is not added.
//
// vs_inflate_block_probe.  ONE WORKGROUP OF ONE WAVE PER CANDIDATE, control flow wave-uniform as in inflate_segments_kernel.  In LDS (about
// 67.5 KiB: two workgroups per CU): the code tables and a RING of 32768 cells of 16 bits, so the output of a span is not capped; a match is
// copied by all lanes, LDS operations of a wave execute in program order and a wave-scope fence keeps the compiler from reordering across
// the phases.  At the end the wave writes the last min(produced, 32768) cells to the candidate's row and the report words.
//
// vs_inflate_block_windows.  ONE workgroup of 1024 threads, two windows in LDS (64 KiB): per span of the chain the new window is computed
// from the old one and the span's cells, written to LDS and to its row in HBM, one barrier per span.
//
// vs_inflate_block_decode.  One wave per span: vs_inflate_zlib's ring (36 KiB in LDS, flushed in 4 KiB pieces) preloaded with the span's
// window, so that a distance reaches into the bytes before the span without reading the output back.
#include "vs_common.h"

namespace {

__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (int64_t)__shfl_xor((long long)v, o, 64);
    return v;
}

}  // namespace

#define VSI_SYNC() __syncthreads()
#define VSC_FENCE() wave_fence()
#define VSC_WAVE_SUM(v) wave_sum_i(v)
#define VSC_WAVE_MAX(v) wave_max_i(v)
#define VSB_WAVE_SUM64(v) wave_sum_i64(v)
#include "vs_inflate_blocks_core.h"

namespace {

constexpr int SCAN_BYTES = 4;                 // bytes (8 bit positions each) per thread
constexpr int SCAN_BLOCK = 256;
constexpr int WIN_BLOCK = 1024;
constexpr int DEC_RING = 36 * 1024;           // window + room to write ahead, as vs_inflate_zlib
constexpr int DEC_PIECE = 4096;               // bytes per flush; DEC_RING and VSB_WINDOW are multiples, so a piece never wraps
constexpr int DEC_STORED_PIECE = 2048;
static_assert(VSB_WINDOW == 32768 && DEC_RING % DEC_PIECE == 0 && VSB_WINDOW % DEC_PIECE == 0, "pieces of the ring do not wrap");
static_assert(8 * (SCAN_BYTES - 1) + VSB_QUICK_BITS <= 8 * 16, "the 16 bytes a thread reads hold what vsb_quick looks at from its last position");

__global__ __launch_bounds__(SCAN_BLOCK) void block_scan_kernel(const uint8_t* __restrict__ comp, int64_t n, int64_t* __restrict__ cand, int64_t cap,
                                                                unsigned long long* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int64_t p0 = ((int64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x) * SCAN_BYTES;   // this thread owns the positions in bytes p0 .. p0 + 3
    uint64_t lo = 0, mid = 0;                                               // bytes p0 .. p0 + 15, zeros beyond the end
    if (p0 + 16 <= n && (((uintptr_t)(comp + p0)) & 3) == 0) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(comp + p0);
        lo = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
        mid = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (p0 + k < n) lo |= (uint64_t)comp[p0 + k] << (8 * k);
            if (p0 + 8 + k < n) mid |= (uint64_t)comp[p0 + 8 + k] << (8 * k);
        }
    }
    uint32_t quick = 0;
#pragma unroll
    for (int k = 0; k < SCAN_BYTES; ++k) {
        const uint64_t a = k ? (lo >> (8 * k)) | (mid << (64 - 8 * k)) : lo;   // the 64 bits from byte p0 + k, and the 40 behind them
        const uint64_t c = mid >> (8 * k);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const uint64_t w = s ? (a >> s) | (c << (64 - s)) : a;
            if (p0 + k < n && vsb_quick(w, (uint32_t)(c >> s))) quick |= 1u << (8 * k + s);
        }
    }
    uint32_t hits = p0 == 0 ? 1u : 0u;                                      // bit 0 is always a candidate
    while (quick) {                                                         // the survivors of this thread, the lanes side by side
        const int q = __ffs((int)quick) - 1;
        quick &= quick - 1;
        if (vsb_block_start(comp, n, p0 * 8 + q)) hits |= 1u << q;
    }
    const int mine = __popc(hits);
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    const int total = __shfl(incl, 63, 64);
    if (total == 0) return;                                                 // wave-uniform
    unsigned long long base = 0;
    if (lane == 63) base = atomicAdd(count, (unsigned long long)total);
    base = (unsigned long long)__shfl((long long)base, 63, 64);
    int64_t at = (int64_t)base + incl - mine;
    while (hits) {
        const int q = __ffs((int)hits) - 1;
        hits &= hits - 1;
        if (cand && at < cap) cand[at] = p0 * 8 + q;
        ++at;
    }
}

// The stored finder: a thread owns the byte boundaries p0 .. p0 + 3 and reads bytes p0 - 4 .. p0 + 7 (three aligned words, or byte by byte
// at either end of the stream and for a stream that is not word-aligned): LEN and NLEN of boundary B in bytes B .. B + 3, the zero bits in
// front of it in bytes B - 2 and B - 1.  Bytes before the stream count as ones (no candidate has a negative position), bytes behind it
// are never part of a boundary (vsb_stored_boundary's B + 4 <= n).  No LDS, a handful of registers; the list is appended to as above.
__global__ __launch_bounds__(SCAN_BLOCK) void block_scan_stored_kernel(const uint8_t* __restrict__ comp, int64_t n, int64_t* __restrict__ cand, int64_t cap,
                                                                       unsigned long long* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int64_t p0 = ((int64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x) * SCAN_BYTES;
    uint32_t prev = 0xffffffffu, cur = 0, next = 0;                         // bytes p0 - 4 .. p0 - 1, p0 .. p0 + 3, p0 + 4 .. p0 + 7
    if (p0 >= 4 && p0 + 8 <= n && (((uintptr_t)(comp + p0)) & 3) == 0) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(comp + p0);
        prev = w[-1];
        cur = w[0];
        next = w[1];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (p0 - 4 + k >= 0 && p0 - 4 + k < n) prev = (prev & ~(0xffu << (8 * k))) | ((uint32_t)comp[p0 - 4 + k] << (8 * k));
            if (p0 + k < n) cur |= (uint32_t)comp[p0 + k] << (8 * k);
            if (p0 + 4 + k < n) next |= (uint32_t)comp[p0 + 4 + k] << (8 * k);
        }
    }
    const uint64_t before = (uint64_t)prev | ((uint64_t)cur << 32), behind = (uint64_t)cur | ((uint64_t)next << 32);
    uint32_t counts = 0;                                                    // 4 bits per boundary: how many candidates it gives, 0 .. 8
    int mine = 0;
#pragma unroll
    for (int k = 0; k < SCAN_BYTES; ++k) {
        const int64_t B = p0 + k;
        const uint32_t hdr = (uint32_t)(behind >> (8 * k));                 // LEN in the low half, NLEN in the high half
        const bool boundary = B + 4 <= n && ((hdr ^ 0xffffu) & 0xffffu) == (hdr >> 16) && B + 4 + (int64_t)(hdr & 0xffffu) < n;
        const int c = boundary ? vsb_stored_count((uint32_t)(before >> (8 * (k + 2))) & 0xffffu) : 0;
        counts |= (uint32_t)c << (4 * k);
        mine += c;
    }
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    const int total = __shfl(incl, 63, 64);
    if (total == 0) return;                                                 // wave-uniform
    unsigned long long base = 0;
    if (lane == 63) base = atomicAdd(count, (unsigned long long)total);
    base = (unsigned long long)__shfl((long long)base, 63, 64);
    int64_t at = (int64_t)base + incl - mine;
    if (!cand) return;
#pragma unroll
    for (int k = 0; k < SCAN_BYTES; ++k) {
        const int c = (int)((counts >> (4 * k)) & 15u);
        for (int j = 0; j < c; ++j, ++at)
            if (at < cap) cand[at] = (p0 + k) * 8 - 3 - j;
    }
}

__global__ __launch_bounds__(64) void block_probe_kernel(const uint8_t* __restrict__ comp, int64_t comp_bytes, const int64_t* __restrict__ cand,
                                                         int64_t n_cand, int64_t first, uint16_t* __restrict__ cells, int64_t* __restrict__ words) {
    __shared__ VsiTables tables;
    __shared__ __attribute__((aligned(16))) uint16_t ring[VSB_WINDOW];
    const int64_t row = blockIdx.x;
    const int lane = threadIdx.x;
    VscReport r;
    vsb_probe(comp, comp_bytes, cand[first + row], cand, n_cand, &tables, ring, cells + row * (int64_t)VSB_WINDOW, &r, lane, 64);
    if (lane < VS_INFLATE_REPORT_WORDS) {
        const int64_t v = lane == 0 ? r.status : lane == 1 ? r.end : lane == 2 ? r.final : lane == 3 ? r.produced : lane == 4 ? r.externals : r.reach;
        words[row * VS_INFLATE_REPORT_WORDS + lane] = v;
    }
}

__global__ __launch_bounds__(WIN_BLOCK) void block_windows_kernel(const uint16_t* __restrict__ cells, int64_t n_slots, const int64_t* __restrict__ slot_index,
                                                                  const int64_t* __restrict__ produced, int64_t n, uint8_t* windows) {
    __shared__ __attribute__((aligned(16))) uint8_t w[2][VSB_WINDOW];
    const int t = threadIdx.x;
    for (int i = t; i < VSB_WINDOW / 16; i += WIN_BLOCK) reinterpret_cast<u32x4*>(w[0])[i] = reinterpret_cast<const u32x4*>(windows)[i];
    __syncthreads();
    for (int64_t k = 0; k < n; ++k) {                                       // chain order; everything here is uniform over the workgroup
        const int64_t slot = slot_index[k];
        const bool ok = slot >= 0 && slot < n_slots && produced[k] >= 0;
        const int64_t p = ok ? produced[k] : 0;                             // a span out of bounds passes the window on
        const uint16_t* tail = cells + (ok ? slot : 0) * (int64_t)VSB_WINDOW;
        const uint8_t* W = w[k & 1];
        uint8_t* N = w[(k + 1) & 1];
        uint8_t* row = windows + (k + 1) * (int64_t)VSB_WINDOW;
#pragma unroll 2
        for (int e = 0; e < VSB_WINDOW / (4 * WIN_BLOCK); ++e) {
            const int j = 4 * (e * WIN_BLOCK + t);
            uint32_t v = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) v |= (uint32_t)vsb_window_byte(W, tail, p, j + q) << (8 * q);
            *reinterpret_cast<uint32_t*>(N + j) = v;
            *reinterpret_cast<uint32_t*>(row + j) = v;
        }
        __syncthreads();                                                    // the next span reads N; nobody reads W any more
    }
}

// The decode's sink: the ring in LDS, preloaded with the window, flushed to out piece by piece.  Ring index of output byte q: (VSB_WINDOW + q) %
// DEC_RING; the window's byte j is at ring index j.
struct WindowSink {
    uint8_t* ring;
    uint8_t* out;                             // the span's first output byte
    int lane, nlanes;
    int64_t pos, flushed;                     // flushed: a multiple of DEC_PIECE
    int rp;

    // bytes [flushed, flushed + len) of the span, len <= DEC_PIECE, contiguous in the ring; the destination in words where it allows
    __device__ void flush(int len) {
        wave_fence();
        const uint8_t* src = ring + (int)((VSB_WINDOW + flushed) % DEC_RING);
        uint8_t* dst = out + flushed;
        int head = (int)((4 - ((uintptr_t)dst & 3)) & 3);
        if (head > len) head = len;
        if (lane < head) dst[lane] = src[lane];
        const int nw = (len - head) >> 2;
        for (int wd = lane; wd < nw; wd += 64) {
            const uint8_t* p = src + head + 4 * wd;
            reinterpret_cast<uint32_t*>(dst + head)[wd] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        }
        for (int i = head + 4 * nw + lane; i < len; i += 64) dst[i] = src[i];
        flushed += len;
    }
    __device__ void advance(int len) {
        pos += len;
        rp += len;
        if (rp >= DEC_RING) rp -= DEC_RING;
        if (pos - flushed >= DEC_PIECE) flush(DEC_PIECE);
    }
    __device__ void lit(uint8_t v) {
        if (lane == 0) ring[rp] = v;
        advance(1);
    }
    __device__ void copy(int dist, int len) {  // 1 <= dist <= min(pos + hist, 32768), 3 <= len <= 258
        int sp = rp - dist;
        if (sp < 0) sp += DEC_RING;
        wave_fence();
        if (dist >= 64) {
            for (int j = 0; j < len; j += 64) {
                const int i = j + lane;
                if (i < len) {
                    int s = sp + i, d = rp + i;
                    if (s >= DEC_RING) s -= DEC_RING;
                    if (d >= DEC_RING) d -= DEC_RING;
                    ring[d] = ring[s];
                }
                wave_fence();
            }
        } else {
            for (int j = 0; j < len; j += 64) {
                const int i = j + lane;
                if (i < len) {
                    int s = sp + (int)((unsigned)i % (unsigned)dist), d = rp + i;
                    if (s >= DEC_RING) s -= DEC_RING;
                    if (d >= DEC_RING) d -= DEC_RING;
                    ring[d] = ring[s];
                }
            }
        }
        advance(len);
    }
    __device__ void stored(const uint8_t* src, int len) {
        for (int done = 0; done < len; done += DEC_STORED_PIECE) {        // at most 32 turns
            const int m = len - done < DEC_STORED_PIECE ? len - done : DEC_STORED_PIECE;
            for (int i = lane; i < m; i += 64) {
                int d = rp + i;
                if (d >= DEC_RING) d -= DEC_RING;
                ring[d] = src[done + i];
            }
            advance(m);
        }
    }
};

__global__ __launch_bounds__(64) void block_decode_kernel(const uint8_t* __restrict__ comp, int64_t comp_bytes, const int64_t* __restrict__ start_bits,
                                                          const int64_t* __restrict__ end_bits, const int64_t* __restrict__ offsets,
                                                          const int64_t* __restrict__ sizes, const uint8_t* __restrict__ windows, uint8_t* __restrict__ out,
                                                          int64_t out_bytes, int64_t* __restrict__ words) {
    __shared__ VsiTables tables;
    __shared__ __attribute__((aligned(16))) uint8_t ring[DEC_RING];
    const int64_t k = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t off = offsets[k], size = sizes[k];
    VscReport r;
    r.status = VS_INFLATE_OUT_LONG; r.end = start_bits[k]; r.produced = 0;
    if (off >= 0 && size >= 0 && off <= out_bytes - size) {                 // uniform
        const u32x4* win = reinterpret_cast<const u32x4*>(windows + k * (int64_t)VSB_WINDOW);
        for (int i = lane; i < VSB_WINDOW / 16; i += 64) reinterpret_cast<u32x4*>(ring)[i] = win[i];
        wave_fence();
        WindowSink sink;
        sink.ring = ring; sink.out = out + off; sink.lane = lane; sink.nlanes = 64;
        sink.pos = 0; sink.flushed = 0; sink.rp = VSB_WINDOW;
        vsb_inflate_span(comp, comp_bytes, start_bits[k], (const int64_t*)nullptr, (int64_t)0, end_bits[k], size,
                         off < VSB_WINDOW ? off : (int64_t)VSB_WINDOW, &tables, sink, &r);
        if (sink.pos > sink.flushed) sink.flush((int)(sink.pos - sink.flushed));   // also what was produced before a failure: inside the span's bytes
    }
    if (lane < VS_INFLATE_DECODE_WORDS) words[k * VS_INFLATE_DECODE_WORDS + lane] = lane == 0 ? r.status : lane == 1 ? r.end : r.produced;
}

}  // namespace

extern "C" int vs_inflate_block_scan(const uint8_t* comp, int64_t comp_bytes, int64_t* cand, int64_t cap, int64_t* count, void* stream) {
    VS_CHECK_ARG(comp && count, "vs_inflate_block_scan: null pointer");
    VS_CHECK_ARG(comp_bytes >= 0 && cap >= 0, "vs_inflate_block_scan: comp_bytes %lld and cap %lld must not be negative", (long long)comp_bytes,
                 (long long)cap);
    VS_CHECK_ARG(cand || cap == 0, "vs_inflate_block_scan: a null list needs cap 0 (got %lld)", (long long)cap);
    const int64_t per_block = (int64_t)SCAN_BLOCK * SCAN_BYTES;
    const int64_t blocks = comp_bytes / per_block + 1;                      // at least one: bit 0 is a candidate of an empty stream too
    VS_CHECK_ARG(blocks <= 2147483647ll, "vs_inflate_block_scan: %lld bytes exceed the grid limit", (long long)comp_bytes);
    hipLaunchKernelGGL(block_scan_kernel, dim3((unsigned)blocks), dim3(SCAN_BLOCK), 0, (hipStream_t)stream, comp, comp_bytes, cand, cap,
                       reinterpret_cast<unsigned long long*>(count));
    VS_CHECK_LAUNCH("vs_inflate_block_scan");
    return VS_OK;
}

extern "C" int vs_inflate_block_scan_stored(const uint8_t* comp, int64_t comp_bytes, int64_t* cand, int64_t cap, int64_t* count, void* stream) {
    VS_CHECK_ARG(comp && count, "vs_inflate_block_scan_stored: null pointer");
    VS_CHECK_ARG(comp_bytes >= 0 && cap >= 0, "vs_inflate_block_scan_stored: comp_bytes %lld and cap %lld must not be negative", (long long)comp_bytes,
                 (long long)cap);
    VS_CHECK_ARG(cand || cap == 0, "vs_inflate_block_scan_stored: a null list needs cap 0 (got %lld)", (long long)cap);
    const int64_t per_block = (int64_t)SCAN_BLOCK * SCAN_BYTES;
    const int64_t blocks = comp_bytes / per_block + 1;
    VS_CHECK_ARG(blocks <= 2147483647ll, "vs_inflate_block_scan_stored: %lld bytes exceed the grid limit", (long long)comp_bytes);
    if (comp_bytes < 5) return VS_OK;                                       // no room for LEN, NLEN and a byte behind them: nothing launched
    hipLaunchKernelGGL(block_scan_stored_kernel, dim3((unsigned)blocks), dim3(SCAN_BLOCK), 0, (hipStream_t)stream, comp, comp_bytes, cand, cap,
                       reinterpret_cast<unsigned long long*>(count));
    VS_CHECK_LAUNCH("vs_inflate_block_scan_stored");
    return VS_OK;
}

extern "C" int vs_inflate_block_probe(const uint8_t* comp, int64_t comp_bytes, const int64_t* cand, int64_t n_cand, int64_t first, int64_t n,
                                      uint16_t* cells, int64_t* words, void* stream) {
    VS_CHECK_ARG(comp && cand && cells && words, "vs_inflate_block_probe: null pointer");
    VS_CHECK_ARG(comp_bytes >= 0 && n_cand >= 0 && first >= 0 && n >= 0,
                 "vs_inflate_block_probe: comp_bytes %lld, n_cand %lld, first %lld and n %lld must not be negative", (long long)comp_bytes,
                 (long long)n_cand, (long long)first, (long long)n);
    VS_CHECK_ARG(n <= VS_INFLATE_MAX_BATCH, "vs_inflate_block_probe: a batch of %lld candidates exceeds the grid limit %lld", (long long)n,
                 (long long)VS_INFLATE_MAX_BATCH);
    VS_CHECK_ARG(first <= n_cand - n, "vs_inflate_block_probe: candidates %lld .. %lld of a list of %lld", (long long)first, (long long)(first + n),
                 (long long)n_cand);
    VS_CHECK_ARG(((uintptr_t)cells & 1) == 0, "vs_inflate_block_probe: cells %p is not at a 2-byte boundary", (void*)cells);
    if (n == 0) return VS_OK;
    hipLaunchKernelGGL(block_probe_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, comp, comp_bytes, cand, n_cand, first, cells, words);
    VS_CHECK_LAUNCH("vs_inflate_block_probe");
    return VS_OK;
}

extern "C" int vs_inflate_block_windows(const uint16_t* cells, int64_t n_slots, const int64_t* slot_index, const int64_t* produced, int64_t n,
                                        uint8_t* windows, void* stream) {
    VS_CHECK_ARG(cells && slot_index && produced && windows, "vs_inflate_block_windows: null pointer");
    VS_CHECK_ARG(n >= 0 && n_slots >= 0, "vs_inflate_block_windows: n %lld and n_slots %lld must not be negative", (long long)n, (long long)n_slots);
    VS_CHECK_ARG(n <= VS_INFLATE_MAX_BATCH && n_slots <= VS_INFLATE_MAX_BATCH, "vs_inflate_block_windows: %lld spans of %lld slots exceed the limit %lld",
                 (long long)n, (long long)n_slots, (long long)VS_INFLATE_MAX_BATCH);
    VS_CHECK_ARG(((uintptr_t)cells & 1) == 0, "vs_inflate_block_windows: cells %p is not at a 2-byte boundary", (void*)cells);
    VS_CHECK_ARG(((uintptr_t)windows & 15) == 0, "vs_inflate_block_windows: windows %p is not at a 16-byte boundary", (void*)windows);
    if (n == 0) return VS_OK;
    hipLaunchKernelGGL(block_windows_kernel, dim3(1), dim3(WIN_BLOCK), 0, (hipStream_t)stream, cells, n_slots, slot_index, produced, n, windows);
    VS_CHECK_LAUNCH("vs_inflate_block_windows");
    return VS_OK;
}

extern "C" int vs_inflate_block_decode(const uint8_t* comp, int64_t comp_bytes, const int64_t* start_bits, const int64_t* end_bits, const int64_t* offsets,
                                       const int64_t* sizes, int64_t n, const uint8_t* windows, uint8_t* out, int64_t out_bytes, int64_t* words,
                                       void* stream) {
    VS_CHECK_ARG(comp && start_bits && end_bits && offsets && sizes && windows && out && words, "vs_inflate_block_decode: null pointer");
    VS_CHECK_ARG(comp_bytes >= 0 && n >= 0 && out_bytes >= 0, "vs_inflate_block_decode: comp_bytes %lld, n %lld and out_bytes %lld must not be negative",
                 (long long)comp_bytes, (long long)n, (long long)out_bytes);
    VS_CHECK_ARG(n <= VS_INFLATE_MAX_BATCH, "vs_inflate_block_decode: %lld spans exceed the grid limit %lld", (long long)n, (long long)VS_INFLATE_MAX_BATCH);
    VS_CHECK_ARG(((uintptr_t)windows & 15) == 0, "vs_inflate_block_decode: windows %p is not at a 16-byte boundary", (void*)windows);
    if (n == 0) return VS_OK;
    hipLaunchKernelGGL(block_decode_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, comp, comp_bytes, start_bits, end_bits, offsets, sizes,
                       windows, out, out_bytes, words);
    VS_CHECK_LAUNCH("vs_inflate_block_decode");
    return VS_OK;
}

// vs_inflate_chunks.hip -- chunk-parallel DEFLATE decoding on the device, the reader of the .npz members that csrc/vs_deflate.hip writes:
// vs_inflate_sync_scan (where segments may start), vs_inflate_segments (one wave per candidate start), vs_inflate_place (the segments of the
// chain into the output) and vs_inflate_resolve (the bytes whose source lies before their segment).  A member is a raw RFC 1951 stream cut
// at byte-aligned empty stored blocks (00 00 FF FF); no index is stored, the markers are found.  The host walks the chain of segments from
// offset 0 over the small report table (ops.inflate_raw); no kernel waits on another workgroup: order comes from launch order and from
// the single workgroup of vs_inflate_resolve.
//
// vs_inflate_sync_scan.  Memory-rate work over the compressed bytes: a thread owns 16 positions p (one 16-byte load + the three bytes
// behind), a wave appends its matches p + 4 to the list with one atomic per wave.  The list is unordered; the count goes on past the
// capacity so that the caller learns the size it needs.
//
// vs_inflate_segments.  The logic is csrc/vs_inflate_chunks_core.h, which also runs on the CPU.  ONE WORKGROUP OF ONE WAVE PER CANDIDATE,
// control flow wave-uniform as in inflate_zlib_kernel.  In LDS (about 67.5 KiB: two workgroups per CU): the code tables (3.5 KiB) and the
// segment's 32768 CELLS of 16 bits -- a byte's value, or the mark of an external byte.  A match is copied by all lanes; LDS operations of a
// wave execute in program order and a wave-scope fence keeps the compiler from reordering across the phases.  At the end the wave writes
// the values to the candidate's slot, the marks (o + 1, 0 for a value) only when the segment has externals, and the report words.
//
// vs_inflate_place.  One workgroup per chain segment, the mirror of vs_deflate_pack: slot -> out + offset, the destination in words.
//
// vs_inflate_resolve.  ONE workgroup walks the listed segments (those with externals) in chain order: out[S + i] = out[S - mark] for every
// marked i, one barrier per segment.  A source lies before S: it was placed by the launch before, or filled for an earlier segment.
#include "vs_common.h"

namespace {

__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

}  // namespace

#define VSI_SYNC() __syncthreads()
#define VSC_FENCE() wave_fence()
#define VSC_WAVE_SUM(v) wave_sum_i(v)
#define VSC_WAVE_MAX(v) wave_max_i(v)
#include "vs_inflate_chunks_core.h"

namespace {

constexpr int SCAN_PER_THREAD = 16;
constexpr int SCAN_BLOCK = 256;
constexpr int RESOLVE_BLOCK = 1024;
static_assert(VSC_MAX_OUT == VS_INFLATE_SLOT_BYTES, "a slot holds a whole segment");

__global__ __launch_bounds__(SCAN_BLOCK) void sync_scan_kernel(const uint8_t* __restrict__ comp, int64_t n, int64_t* __restrict__ cand, int64_t cap,
                                                               unsigned long long* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int64_t p0 = ((int64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x) * SCAN_PER_THREAD;   // this thread owns the matches that START at p0 .. p0 + 15
    uint8_t v[SCAN_PER_THREAD + 3];
    if (p0 + SCAN_PER_THREAD + 3 <= n && (((uintptr_t)(comp + p0)) & 15) == 0) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(comp + p0);
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
#pragma unroll
        for (int k = 16; k < 19; ++k) v[k] = comp[p0 + k];
    } else {
#pragma unroll
        for (int k = 0; k < SCAN_PER_THREAD + 3; ++k) v[k] = p0 + k < n ? comp[p0 + k] : (uint8_t)1;   // 1 is no byte of the marker
    }
    uint32_t hits = 0;
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD; ++k)
        if (v[k] == 0 && v[k + 1] == 0 && v[k + 2] == 0xFF && v[k + 3] == 0xFF && p0 + k + 4 <= n) hits |= 1u << k;
    int mine = __popc(hits) + (p0 == 0 ? 1 : 0);                            // offset 0 is always a candidate
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
    if (p0 == 0) {
        if (cand && at < cap) cand[at] = 0;
        ++at;
    }
    for (int k = 0; k < SCAN_PER_THREAD; ++k)
        if (hits & (1u << k)) {
            if (cand && at < cap) cand[at] = p0 + k + 4;
            ++at;
        }
}

__global__ __launch_bounds__(64) void inflate_segments_kernel(const uint8_t* __restrict__ comp, int64_t comp_bytes, const int64_t* __restrict__ cand,
                                                              uint8_t* __restrict__ slots, int64_t slot_stride, uint16_t* __restrict__ marks,
                                                              int64_t* __restrict__ words) {
    __shared__ VsiTables tables;
    __shared__ __attribute__((aligned(16))) uint16_t cell[VSC_MAX_OUT];
    const int64_t c = blockIdx.x;
    const int lane = threadIdx.x;
    VscReport r;
    vsc_inflate_segment(comp, comp_bytes, cand[c], &tables, cell, &r, lane, 64);
    wave_fence();
    const int n = (int)r.produced;                                          // <= VSC_MAX_OUT <= slot_stride
    if (r.status == VS_INFLATE_OK) {
        uint8_t* slot = slots + c * slot_stride;
        int done = 0;
        if (((uintptr_t)slot & 3) == 0) {
            const int full = n >> 2;
            for (int w = lane; w < full; w += 64) {
                const uint16_t* s = cell + 4 * w;
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) v |= ((s[k] & VSC_EXT) ? 0u : (uint32_t)(s[k] & 255u)) << (8 * k);
                reinterpret_cast<uint32_t*>(slot)[w] = v;
            }
            done = full << 2;
        }
        for (int i = done + lane; i < n; i += 64) slot[i] = (cell[i] & VSC_EXT) ? (uint8_t)0 : (uint8_t)cell[i];
        if (r.externals > 0) {                                              // marks: o + 1 for an external byte, 0 for a value
            uint16_t* m = marks + c * (int64_t)VSC_MAX_OUT;
            for (int i = lane; i < n; i += 64) m[i] = (cell[i] & VSC_EXT) ? (uint16_t)((cell[i] & 0x7fffu) + 1u) : (uint16_t)0;
        }
    }
    if (lane < VS_INFLATE_REPORT_WORDS) {
        const int64_t v = lane == 0 ? r.status : lane == 1 ? r.end : lane == 2 ? r.final : lane == 3 ? r.produced : lane == 4 ? r.externals : r.reach;
        words[c * VS_INFLATE_REPORT_WORDS + lane] = v;
    }
}

__global__ __launch_bounds__(256) void inflate_place_kernel(const uint8_t* __restrict__ slots, int64_t slot_stride, int64_t n_slots,
                                                            const int64_t* __restrict__ slot_index, const int64_t* __restrict__ sizes,
                                                            const int64_t* __restrict__ offsets, uint8_t* __restrict__ out, int64_t out_bytes) {
    const int64_t c = blockIdx.x, slot = slot_index[c], size = sizes[c], off = offsets[c];
    if (slot < 0 || slot >= n_slots || size < 0 || size > VSC_MAX_OUT || off < 0 || off > out_bytes - size) return;
    const uint8_t* s = slots + slot * slot_stride;
    uint8_t* d = out + off;
    int64_t head = (int64_t)((4 - ((uintptr_t)d & 3)) & 3);                 // the destination in words; the source by bytes (it is in cache)
    if (head > size) head = size;
    if ((int64_t)threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
    const int64_t nw = (size - head) >> 2;
    for (int64_t wd = threadIdx.x; wd < nw; wd += 256) {
        const uint8_t* p = s + head + 4 * wd;
        reinterpret_cast<uint32_t*>(d + head)[wd] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    }
    for (int64_t i = head + 4 * nw + threadIdx.x; i < size; i += 256) d[i] = s[i];
}

__global__ __launch_bounds__(RESOLVE_BLOCK) void inflate_resolve_kernel(const uint16_t* __restrict__ marks, int64_t n_slots,
                                                                        const int64_t* __restrict__ slot_index, const int64_t* __restrict__ sizes,
                                                                        const int64_t* __restrict__ offsets, int64_t n, uint8_t* out, int64_t out_bytes) {
    for (int64_t c = 0; c < n; ++c) {                                       // chain order; everything here is uniform over the workgroup
        const int64_t slot = slot_index[c], size = sizes[c], off = offsets[c];
        if (!(slot < 0 || slot >= n_slots || size < 0 || size > VSC_MAX_OUT || off < 0 || off > out_bytes - size)) {
            const uint16_t* m = marks + slot * (int64_t)VSC_MAX_OUT;
            for (int i = threadIdx.x; i < (int)size; i += RESOLVE_BLOCK) {
                const int64_t mark = m[i];
                if (mark != 0 && mark <= off) out[off + i] = out[off - mark];    // the source lies before this segment: final already
            }
        }
        __syncthreads();                                                    // (with its workgroup-scope fence) the next segment reads what this one filled
    }
}

}  // namespace

extern "C" int vs_inflate_sync_scan(const uint8_t* comp, int64_t comp_bytes, int64_t* cand, int64_t cap, int64_t* count, void* stream) {
    VS_CHECK_ARG(comp && count, "vs_inflate_sync_scan: null pointer");
    VS_CHECK_ARG(comp_bytes >= 0 && cap >= 0, "vs_inflate_sync_scan: comp_bytes %lld and cap %lld must not be negative", (long long)comp_bytes,
                 (long long)cap);
    VS_CHECK_ARG(cand || cap == 0, "vs_inflate_sync_scan: a null list needs cap 0 (got %lld)", (long long)cap);
    const int64_t per_block = (int64_t)SCAN_BLOCK * SCAN_PER_THREAD;
    const int64_t blocks = comp_bytes / per_block + 1;                      // at least one: offset 0 is a candidate of an empty stream too
    VS_CHECK_ARG(blocks <= 2147483647ll, "vs_inflate_sync_scan: %lld bytes exceed the grid limit", (long long)comp_bytes);
    hipLaunchKernelGGL(sync_scan_kernel, dim3((unsigned)blocks), dim3(SCAN_BLOCK), 0, (hipStream_t)stream, comp, comp_bytes, cand, cap,
                       reinterpret_cast<unsigned long long*>(count));
    VS_CHECK_LAUNCH("vs_inflate_sync_scan");
    return VS_OK;
}

extern "C" int vs_inflate_segments(const uint8_t* comp, int64_t comp_bytes, const int64_t* cand, int64_t n_cand, uint8_t* slots, int64_t slot_stride,
                                   uint16_t* marks, int64_t* words, void* stream) {
    VS_CHECK_ARG(comp && cand && slots && marks && words, "vs_inflate_segments: null pointer");
    VS_CHECK_ARG(comp_bytes >= 0 && n_cand >= 0, "vs_inflate_segments: comp_bytes %lld and n_cand %lld must not be negative", (long long)comp_bytes,
                 (long long)n_cand);
    VS_CHECK_ARG(n_cand <= VS_INFLATE_MAX_BATCH, "vs_inflate_segments: a batch of %lld candidates exceeds the grid limit %lld", (long long)n_cand,
                 (long long)VS_INFLATE_MAX_BATCH);
    VS_CHECK_ARG(slot_stride >= VS_INFLATE_SLOT_BYTES, "vs_inflate_segments: slot_stride %lld is below %d", (long long)slot_stride, VS_INFLATE_SLOT_BYTES);
    VS_CHECK_ARG(((uintptr_t)marks & 1) == 0, "vs_inflate_segments: marks %p is not at a 2-byte boundary", (void*)marks);
    if (n_cand == 0) return VS_OK;
    hipLaunchKernelGGL(inflate_segments_kernel, dim3((unsigned)n_cand), dim3(64), 0, (hipStream_t)stream, comp, comp_bytes, cand, slots, slot_stride, marks,
                       words);
    VS_CHECK_LAUNCH("vs_inflate_segments");
    return VS_OK;
}

extern "C" int vs_inflate_place(const uint8_t* slots, int64_t slot_stride, int64_t n_slots, const int64_t* slot_index, const int64_t* sizes,
                                const int64_t* offsets, int64_t n, uint8_t* out, int64_t out_bytes, void* stream) {
    VS_CHECK_ARG(slots && slot_index && sizes && offsets && out, "vs_inflate_place: null pointer");
    VS_CHECK_ARG(n >= 0 && n_slots >= 0 && out_bytes >= 0, "vs_inflate_place: n %lld, n_slots %lld and out_bytes %lld must not be negative", (long long)n,
                 (long long)n_slots, (long long)out_bytes);
    VS_CHECK_ARG(n <= VS_INFLATE_MAX_BATCH && n_slots <= VS_INFLATE_MAX_BATCH, "vs_inflate_place: %lld segments of %lld slots exceed the grid limit %lld",
                 (long long)n, (long long)n_slots, (long long)VS_INFLATE_MAX_BATCH);
    VS_CHECK_ARG(slot_stride >= VS_INFLATE_SLOT_BYTES, "vs_inflate_place: slot_stride %lld is below %d", (long long)slot_stride, VS_INFLATE_SLOT_BYTES);
    if (n == 0) return VS_OK;
    hipLaunchKernelGGL(inflate_place_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, slots, slot_stride, n_slots, slot_index, sizes, offsets,
                       out, out_bytes);
    VS_CHECK_LAUNCH("vs_inflate_place");
    return VS_OK;
}

extern "C" int vs_inflate_resolve(const uint16_t* marks, int64_t n_slots, const int64_t* slot_index, const int64_t* sizes, const int64_t* offsets,
                                  int64_t n, uint8_t* out, int64_t out_bytes, void* stream) {
    VS_CHECK_ARG(marks && slot_index && sizes && offsets && out, "vs_inflate_resolve: null pointer");
    VS_CHECK_ARG(n >= 0 && n_slots >= 0 && out_bytes >= 0, "vs_inflate_resolve: n %lld, n_slots %lld and out_bytes %lld must not be negative", (long long)n,
                 (long long)n_slots, (long long)out_bytes);
    VS_CHECK_ARG(n <= VS_INFLATE_MAX_BATCH && n_slots <= VS_INFLATE_MAX_BATCH, "vs_inflate_resolve: %lld segments of %lld slots exceed the grid limit %lld",
                 (long long)n, (long long)n_slots, (long long)VS_INFLATE_MAX_BATCH);
    VS_CHECK_ARG(((uintptr_t)marks & 1) == 0, "vs_inflate_resolve: marks %p is not at a 2-byte boundary", (void*)marks);
    if (n == 0) return VS_OK;
    hipLaunchKernelGGL(inflate_resolve_kernel, dim3(1), dim3(RESOLVE_BLOCK), 0, (hipStream_t)stream, marks, n_slots, slot_index, sizes, offsets, n, out,
                       out_bytes);
    VS_CHECK_LAUNCH("vs_inflate_resolve");
    return VS_OK;
}

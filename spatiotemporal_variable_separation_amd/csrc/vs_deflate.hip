// vs_deflate.hip -- DEFLATE compression on the device: vs_deflate_chunks (one wave per independent chunk), vs_deflate_pack (the used part of
// every slot into one buffer) and vs_crc32 (the CRC a zip member needs, piecewise).  An array that is already in HBM -- the Moving-MNIST
// test videos -- is compressed where it lies; only the compressed bytes cross to the host, which writes them into the .npz member.
//
// vs_deflate_chunks.  The logic (runs, tokens, code construction, the choice among stored / fixed / dynamic by exact bits, header, emission)
// is csrc/vs_deflate_core.h, which also runs on the CPU; this file adds the wave primitives and the moves between HBM and LDS.  ONE
// WORKGROUP OF ONE WAVE PER CHUNK of at most 32 KiB.  Per workgroup, in LDS (about 73 KiB: two workgroups per CU of 160 KiB):
//   * the chunk, staged with 16-byte loads (byte loads up to the first and after the last 16-byte boundary of the source), at the source's
//     own offset inside a 16-byte line;
//   * the run-start mask (one bit per position: 64 positions per __ballot), histogram, code tables and header scratch (VsdWork, 8.5 KiB);
//   * the image of the chunk's output.  Each lane encodes the token that starts at its position; a wave prefix sum of the bit lengths
//     gives every lane its bit offset and the bits are OR-ed into the image with LDS atomics.  A window of 64 background positions (no
//     run starts, no 258-piece starts) is recognised from the mask alone and skipped.
// The image is written to the slot with 16-byte stores when the slot is aligned so, by bytes otherwise; only the chunk's own byte count
// is written, and that count is at most chunk length + VS_DEFLATE_SLOT_EXTRA, which the entry point checks against slot_stride.
//
// vs_deflate_chunks_window.  The same chunks, slots and sizes with the WINDOW matcher of csrc/vs_deflate_window_core.h: matches up to 32768
// bytes back, also into the bytes before the chunk.  One workgroup of one wave per CU (about 145 KiB of LDS) loops over chunks:
//   * up to 32 KiB of history and the chunk, staged as above; the image shares its bytes with the history, which is dead after the search;
//   * the hash table of the search (64 KiB, `atomicMax`: the largest position of a block of 64 wins), two VsdWork (the runs parse's and
//     the window parse's) and the distance code;
//   * the per-position (length, distance) words do not fit beside these: they live in the workgroup's own slice of a global workspace.
// The greedy chain through a window of 64 positions is resolved by pointer doubling with wave shuffles (wave_chain).
//
// vs_crc32.  One wave per piece, four waves per workgroup sharing the byte table in LDS.  Each lane takes a sub-piece, computes its plain
// CRC (word loads) and advances it past all bytes behind it by square-and-multiply in GF(2)[x] / P; the lanes' results are XOR-ed.
#include "vs_common.h"

namespace {

__device__ __forceinline__ int wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}
// The greedy chain through a window of 64 positions by pointer doubling: lane k's token, if one starts there, ends at local position
// nx > k (64 and above: outside the window).  bits: the lanes the chain visits from lane `entry` (0..63, uniform) on; out: the first
// position >= 64 it reaches.  After round r a lane knows the next 2^r positions of its own chain, so 6 rounds cover the window.
__device__ __forceinline__ void wave_chain(int nx, int entry, uint64_t& bits, int& out) {
    uint32_t lo = threadIdx.x < 32 ? 1u << (threadIdx.x & 31) : 0u, hi = threadIdx.x < 32 ? 0u : 1u << (threadIdx.x & 31);
    int n = nx;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const int from = n & 63;
        const uint32_t flo = (uint32_t)__shfl((int)lo, from, 64), fhi = (uint32_t)__shfl((int)hi, from, 64);
        const int fn = __shfl(n, from, 64);
        if (n < 64) { lo |= flo; hi |= fhi; n = fn; }
    }
    lo = (uint32_t)__shfl((int)lo, entry, 64);
    hi = (uint32_t)__shfl((int)hi, entry, 64);
    bits = ((uint64_t)hi << 32) | lo;
    out = __shfl(n, entry, 64);
}

}  // namespace

// the wave's forms of the core's primitives (the core is compiled for the device only here)
#define VSD_HD __device__ inline
#define VSD_SYNC() __syncthreads()
#define VSD_BALLOT(p) ((uint64_t)__ballot(p))
#define VSD_SCAN(v, before, total) ((total) = wave_incl_scan(v), (before) = (total) - (v), (total) = __shfl((total), 63, 64))
#define VSD_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#define VSD_ATOMIC_OR(p, v) atomicOr((p), (v))
#define VSW_TABLE_MAX(p, v) atomicMax((p), (v))
#define VSW_CHAIN(nx, entry, bits, out) wave_chain((nx), (entry), (bits), (out))
#include "vs_deflate_window_core.h"

namespace {

constexpr int STAGE_BYTES = VSD_MAX_CHUNK + 16;
constexpr int IMAGE_WORDS = (VSD_MAX_CHUNK + VSD_SLOT_EXTRA + 3) / 4;
// vs_deflate_chunks_window: the image (IMAGE_WORDS rounded up to 16 bytes, below WIN_X_AT) shares its bytes with the history, which is
// dead when the image is first written; the chunk follows at the source's own offset inside a 16-byte line
constexpr int WIN_X_AT = 48 + VSW_MAX_HISTORY;
constexpr int WIN_STAGE_BYTES = WIN_X_AT + 16 + VSD_MAX_CHUNK;
static_assert(WIN_X_AT % 16 == 0 && (IMAGE_WORDS + 3) / 4 * 16 <= WIN_X_AT, "the image ends before the chunk");
static_assert(VS_DEFLATE_WINDOW_GROUP_BYTES == 4 * VSD_MAX_CHUNK, "one word per position of a chunk");

__global__ __launch_bounds__(64) void deflate_chunks_kernel(const uint8_t* __restrict__ src, int64_t n_bytes, int chunk_bytes,
                                                            uint8_t* __restrict__ slots, int64_t slot_stride, int64_t* __restrict__ sizes) {
    __shared__ VsdWork work;
    __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE_BYTES];
    __shared__ __attribute__((aligned(16))) uint32_t image[(IMAGE_WORDS + 3) / 4 * 4];
    const int lane = threadIdx.x;
    const int64_t c = blockIdx.x, lo = c * (int64_t)chunk_bytes;
    const int n = (int)(n_bytes - lo < chunk_bytes ? n_bytes - lo : chunk_bytes);      // 1 .. chunk_bytes: the grid is ceil(n_bytes / chunk_bytes)
    const uint8_t* in = src + lo;
    const int a = (int)((uintptr_t)in & 15);
    uint8_t* x = stage + a;                                                // x + i and in + i share their offset inside a 16-byte line
    int head = (16 - a) & 15;
    if (head > n) head = n;
    const int vecs = (n - head) >> 4;
    if (lane < head) x[lane] = in[lane];
    for (int v = lane; v < vecs; v += 64)
        *reinterpret_cast<u32x4*>(x + head + 16 * v) = *reinterpret_cast<const u32x4*>(in + head + 16 * v);
    for (int i = head + 16 * vecs + lane; i < n; i += 64) x[i] = in[i];     // at most 15 bytes
    const int size = vsd_deflate_chunk(x, n, &work, image, lane, 64);
    uint8_t* slot = slots + c * slot_stride;
    const uint8_t* img = reinterpret_cast<const uint8_t*>(image);
    int done = 0;
    if (((uintptr_t)slot & 15) == 0) {
        const int full = size >> 4;
        for (int v = lane; v < full; v += 64) reinterpret_cast<u32x4*>(slot)[v] = reinterpret_cast<const u32x4*>(image)[v];
        done = full << 4;
    }
    for (int i = done + lane; i < size; i += 64) slot[i] = img[i];
    if (lane == 0) sizes[c] = size;
}

// One workgroup of one wave loops over the chunks c = blockIdx.x, blockIdx.x + gridDim.x, ...; its per-position words are its own
// VS_DEFLATE_WINDOW_GROUP_BYTES of the workspace.  `before` = history_bytes + the chunk's offset is what lies before the chunk in the
// array; the last min(VSW_MAX_HISTORY, before) bytes of it are staged in front of the chunk.
__global__ __launch_bounds__(64) void deflate_chunks_window_kernel(const uint8_t* __restrict__ src, int64_t history_bytes, int64_t n_bytes,
                                                                   int chunk_bytes, int64_t chunks, uint8_t* __restrict__ slots, int64_t slot_stride,
                                                                   int64_t* __restrict__ sizes, uint32_t* __restrict__ workspace) {
    __shared__ VsdWork runs_work;
    __shared__ VsdWork window_work;
    __shared__ VswWork search;
    __shared__ __attribute__((aligned(16))) uint8_t stage[WIN_STAGE_BYTES];
    const int lane = threadIdx.x;
    uint32_t* pk = workspace + (int64_t)blockIdx.x * VSD_MAX_CHUNK;
    uint32_t* image = reinterpret_cast<uint32_t*>(stage);
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t lo = c * (int64_t)chunk_bytes, before = history_bytes + lo;
        const int n = (int)(n_bytes - lo < chunk_bytes ? n_bytes - lo : chunk_bytes);  // 1 .. chunk_bytes
        const int hist = (int)(before < VSW_MAX_HISTORY ? before : VSW_MAX_HISTORY);
        const uint8_t* in = src + lo;
        uint8_t* x = stage + WIN_X_AT + (int)((uintptr_t)in & 15);         // x + i and in + i share their offset inside a 16-byte line
        const uint8_t* g = in - hist;
        uint8_t* y = x - hist;                                              // >= stage + 48
        const int total = hist + n;
        int head = (int)((16 - ((uintptr_t)g & 15)) & 15);
        if (head > total) head = total;
        const int vecs = (total - head) >> 4;
        __syncthreads();                                                    // the previous chunk's image has left the stage
        if (lane < head) y[lane] = g[lane];
        for (int v = lane; v < vecs; v += 64)
            *reinterpret_cast<u32x4*>(y + head + 16 * v) = *reinterpret_cast<const u32x4*>(g + head + 16 * v);
        for (int i = head + 16 * vecs + lane; i < total; i += 64) y[i] = g[i];  // at most 15 bytes
        const int size = vsw_deflate_chunk(x, hist, n, &runs_work, &window_work, &search, pk, image, lane, 64);
        uint8_t* slot = slots + c * slot_stride;
        const uint8_t* img = stage;
        int done = 0;
        if (((uintptr_t)slot & 15) == 0) {
            const int full = size >> 4;
            for (int v = lane; v < full; v += 64) reinterpret_cast<u32x4*>(slot)[v] = reinterpret_cast<const u32x4*>(stage)[v];
            done = full << 4;
        }
        for (int i = done + lane; i < size; i += 64) slot[i] = img[i];
        if (lane == 0) sizes[c] = size;
    }
}

__global__ __launch_bounds__(256) void deflate_pack_kernel(const uint8_t* __restrict__ slots, int64_t slot_stride, const int64_t* __restrict__ sizes,
                                                           const int64_t* __restrict__ offsets, uint8_t* __restrict__ dst, int64_t dst_bytes) {
    const int64_t c = blockIdx.x, size = sizes[c], off = offsets[c];
    if (size < 0 || size > slot_stride || off < 0 || off > dst_bytes - size) return;
    const uint8_t* s = slots + c * slot_stride;
    uint8_t* d = dst + off;
    int64_t head = (int64_t)((4 - ((uintptr_t)d & 3)) & 3);                 // the destination in words; the source by bytes (it is in cache)
    if (head > size) head = size;
    if ((int64_t)threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
    const int64_t words = (size - head) >> 2;
    for (int64_t wd = threadIdx.x; wd < words; wd += 256) {
        const uint8_t* p = s + head + 4 * wd;
        reinterpret_cast<uint32_t*>(d + head)[wd] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    }
    for (int64_t i = head + 4 * words + threadIdx.x; i < size; i += 256) d[i] = s[i];
}

constexpr int CRC_WAVES = 4;

__global__ __launch_bounds__(64 * CRC_WAVES) void crc32_kernel(const uint8_t* __restrict__ src, int64_t n_bytes, int64_t chunk_bytes, uint32_t init,
                                                                uint32_t* __restrict__ partial, int64_t pieces) {
    __shared__ uint32_t table[256];
    table[threadIdx.x] = vsd_crc_table_entry(threadIdx.x);                  // 256 threads, 256 entries
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * CRC_WAVES + (threadIdx.x >> 6);
    if (p >= pieces) return;
    const int64_t lo = p * chunk_bytes, hi = lo + chunk_bytes < n_bytes ? lo + chunk_bytes : n_bytes;
    const uint32_t r = wave_xor(vsd_crc_partial(table, src + lo, n_bytes, lo, hi, init, lane, 64));
    if (lane == 0) partial[p] = r;
}

}  // namespace

extern "C" int vs_deflate_chunks(const uint8_t* src, int64_t n_bytes, int chunk_bytes, uint8_t* slots, int64_t slot_stride, int64_t* sizes,
                                 void* stream) {
    VS_CHECK_ARG(src && slots && sizes, "vs_deflate_chunks: null pointer");
    VS_CHECK_ARG(n_bytes >= 0, "vs_deflate_chunks: n_bytes %lld is negative", (long long)n_bytes);
    VS_CHECK_ARG(chunk_bytes >= VS_DEFLATE_MIN_CHUNK && chunk_bytes <= VS_DEFLATE_MAX_CHUNK, "vs_deflate_chunks: chunk_bytes %d outside %d .. %d",
                 chunk_bytes, VS_DEFLATE_MIN_CHUNK, VS_DEFLATE_MAX_CHUNK);
    VS_CHECK_ARG(slot_stride >= (int64_t)chunk_bytes + VS_DEFLATE_SLOT_EXTRA, "vs_deflate_chunks: slot_stride %lld is below the worst case %d + %d",
                 (long long)slot_stride, chunk_bytes, VS_DEFLATE_SLOT_EXTRA);
    const int64_t chunks = (n_bytes + chunk_bytes - 1) / chunk_bytes;
    VS_CHECK_ARG(chunks <= 2147483647ll, "vs_deflate_chunks: %lld chunks exceed the grid limit", (long long)chunks);
    if (chunks == 0) return VS_OK;
    hipLaunchKernelGGL(deflate_chunks_kernel, dim3((unsigned)chunks), dim3(64), 0, (hipStream_t)stream, src, n_bytes, chunk_bytes, slots, slot_stride,
                       sizes);
    VS_CHECK_LAUNCH("vs_deflate_chunks");
    return VS_OK;
}

extern "C" int vs_deflate_chunks_window(const uint8_t* src, int64_t history_bytes, int64_t n_bytes, int chunk_bytes, uint8_t* slots,
                                        int64_t slot_stride, int64_t* sizes, void* workspace, int64_t workspace_bytes, void* stream) {
    VS_CHECK_ARG(src && slots && sizes, "vs_deflate_chunks_window: null pointer");
    VS_CHECK_ARG(n_bytes >= 0, "vs_deflate_chunks_window: n_bytes %lld is negative", (long long)n_bytes);
    VS_CHECK_ARG(chunk_bytes >= VS_DEFLATE_MIN_CHUNK && chunk_bytes <= VS_DEFLATE_MAX_CHUNK, "vs_deflate_chunks_window: chunk_bytes %d outside %d .. %d",
                 chunk_bytes, VS_DEFLATE_MIN_CHUNK, VS_DEFLATE_MAX_CHUNK);
    VS_CHECK_ARG(slot_stride >= (int64_t)chunk_bytes + VS_DEFLATE_SLOT_EXTRA,
                 "vs_deflate_chunks_window: slot_stride %lld is below the worst case %d + %d", (long long)slot_stride, chunk_bytes, VS_DEFLATE_SLOT_EXTRA);
    VS_CHECK_ARG(history_bytes >= 0 && history_bytes <= VS_DEFLATE_MAX_HISTORY, "vs_deflate_chunks_window: history_bytes %lld outside 0 .. %d",
                 (long long)history_bytes, VS_DEFLATE_MAX_HISTORY);
    const int64_t chunks = (n_bytes + chunk_bytes - 1) / chunk_bytes;
    VS_CHECK_ARG(chunks <= 2147483647ll, "vs_deflate_chunks_window: %lld chunks exceed the grid limit", (long long)chunks);
    VS_CHECK_ARG(workspace && ((uintptr_t)workspace & 3) == 0 && workspace_bytes >= VS_DEFLATE_WINDOW_GROUP_BYTES,
                 "vs_deflate_chunks_window: workspace %p of %lld bytes; %d bytes per workgroup at a 4-byte boundary are needed", workspace,
                 (long long)workspace_bytes, VS_DEFLATE_WINDOW_GROUP_BYTES);
    if (chunks == 0) return VS_OK;
    int64_t groups = workspace_bytes / VS_DEFLATE_WINDOW_GROUP_BYTES;
    if (groups > chunks) groups = chunks;
    hipLaunchKernelGGL(deflate_chunks_window_kernel, dim3((unsigned)groups), dim3(64), 0, (hipStream_t)stream, src, history_bytes, n_bytes, chunk_bytes,
                       chunks, slots, slot_stride, sizes, (uint32_t*)workspace);
    VS_CHECK_LAUNCH("vs_deflate_chunks_window");
    return VS_OK;
}

extern "C" int vs_deflate_pack(const uint8_t* slots, int64_t slot_stride, const int64_t* sizes, const int64_t* offsets, int64_t n_chunks, uint8_t* dst,
                               int64_t dst_bytes, void* stream) {
    VS_CHECK_ARG(slots && sizes && offsets && dst, "vs_deflate_pack: null pointer");
    VS_CHECK_ARG(n_chunks >= 1 && slot_stride >= 1 && dst_bytes >= 0, "vs_deflate_pack: n_chunks %lld and slot_stride %lld must be positive, dst_bytes "
                 "%lld non-negative", (long long)n_chunks, (long long)slot_stride, (long long)dst_bytes);
    VS_CHECK_ARG(n_chunks <= 2147483647ll, "vs_deflate_pack: %lld chunks exceed the grid limit", (long long)n_chunks);
    hipLaunchKernelGGL(deflate_pack_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, slots, slot_stride, sizes, offsets, dst,
                       dst_bytes);
    VS_CHECK_LAUNCH("vs_deflate_pack");
    return VS_OK;
}

extern "C" int vs_crc32(const uint8_t* src, int64_t n_bytes, int64_t chunk_bytes, uint32_t init, uint32_t* partial, void* stream) {
    VS_CHECK_ARG(src && partial, "vs_crc32: null pointer");
    VS_CHECK_ARG(n_bytes >= 0, "vs_crc32: n_bytes %lld is negative", (long long)n_bytes);
    VS_CHECK_ARG(chunk_bytes >= 256 && chunk_bytes <= (1ll << 24), "vs_crc32: chunk_bytes %lld outside 256 .. 2^24", (long long)chunk_bytes);
    const int64_t pieces = (n_bytes + chunk_bytes - 1) / chunk_bytes, blocks = (pieces + CRC_WAVES - 1) / CRC_WAVES;
    VS_CHECK_ARG(blocks <= 2147483647ll, "vs_crc32: %lld pieces exceed the grid limit", (long long)pieces);
    if (pieces == 0) return VS_OK;
    hipLaunchKernelGGL(crc32_kernel, dim3((unsigned)blocks), dim3(64 * CRC_WAVES), 0, (hipStream_t)stream, src, n_bytes, chunk_bytes, init, partial,
                       pieces);
    VS_CHECK_LAUNCH("vs_crc32");
    return VS_OK;
}

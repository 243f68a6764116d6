// vs_png_encode.hip -- PNG encoding on the device: vs_png_filter (pixels into filtered rows), vs_deflate_streams (many equal-length
// streams, each compressed on its own) and vs_png_assemble (one complete file per image).  With vs_inflate_zlib, vs_png_unfilter and
// vs_resample_u8 the chain decode -> resize -> encode stays in HBM: only compressed bytes cross the bus, in both directions.  The logic
// (residuals, the adaptive choice, where a chunk of a stream lies, the framing with its two checksums) is csrc/vs_png_encode_core.h, which
// also runs on the CPU; the DEFLATE of a chunk is csrc/vs_deflate_core.h and csrc/vs_deflate_window_core.h, unchanged.
//
// vs_png_filter.  Encoding has no serial dependency: a residual is a function of four SOURCE bytes.  ONE WAVE PER ROW, FLT_WAVES rows per
// workgroup; the lanes lie along the row, four consecutive bytes per lane, consecutive lanes on consecutive words.  Pass 1 (adaptive mode
// only) walks the row in the word grid of the source row and keeps the five sums of |residual| per lane; one wave reduction gives the
// type.  Pass 2 walks it in the word grid of the DESTINATION (row_bytes + 1 is odd for most shapes: source and destination rarely share
// a grid) and writes one word per lane; the second read of the row comes from cache.  A word of the row, of the row above, and the words
// four bytes before them are one 32-bit load each where that address is aligned and four byte loads where it is not (uniform per row);
// the left and the above-left bytes are a funnel shift of two words by 4 - C bytes.  Bytes before the first and after the last whole word
// are done one per lane.
//
// vs_deflate_streams.  The two kernels of vs_deflate.hip with one change: chunk c = s * K + k is chunk k of stream s, its source is
// src + s * stream_stride + k * chunk_bytes, and the history of the window parse is min(32768, k * chunk_bytes) -- the stream's own bytes.
// Nothing before a stream's first byte is staged, so no match can leave the stream.  Staging, slots and sizes are as there.
//
// vs_png_assemble.  ONE WORKGROUP OF ASM_THREADS PER IMAGE (vpe_assemble).  The IDAT's CRC-32 is computed from the bytes of the file that
// the workgroup has just written: __syncthreads() orders a workgroup's own global writes before its later reads (its waves share one
// CU and one vector L1), and the file is read through the pointer it was written through, without __restrict__.
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
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}
// vs_deflate.hip's wave_chain: the greedy chain through a window of 64 positions by pointer doubling
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

constexpr int ASM_THREADS = 256;
constexpr int ASM_WAVES = ASM_THREADS / 64;

// the sum / the XOR of v over the workgroup of vs_png_assemble, the same in every thread
__device__ __forceinline__ uint32_t group_sum(uint32_t v) {
    __shared__ uint32_t part[ASM_WAVES];
    v = wave_sum(v);
    __syncthreads();                                                        // the previous reduction has been read
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t r = 0;
#pragma unroll
    for (int w = 0; w < ASM_WAVES; ++w) r += part[w];
    return r;
}
__device__ __forceinline__ uint32_t group_xor(uint32_t v) {
    __shared__ uint32_t part[ASM_WAVES];
    v = wave_xor(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t r = 0;
#pragma unroll
    for (int w = 0; w < ASM_WAVES; ++w) r ^= part[w];
    return r;
}

}  // namespace

// the wave's forms of the cores' primitives (the cores are compiled for the device only here), as in vs_deflate.hip
#define VSD_HD __device__ inline
#define VSD_SYNC() __syncthreads()
#define VSD_BALLOT(p) ((uint64_t)__ballot(p))
#define VSD_SCAN(v, before, total) ((total) = wave_incl_scan(v), (before) = (total) - (v), (total) = __shfl((total), 63, 64))
#define VSD_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#define VSD_ATOMIC_OR(p, v) atomicOr((p), (v))
#define VSW_TABLE_MAX(p, v) atomicMax((p), (v))
#define VSW_CHAIN(nx, entry, bits, out) wave_chain((nx), (entry), (bits), (out))
#define VPE_SUM(v) group_sum(v)
#define VPE_XOR(v) group_xor(v)
#include "vs_png_encode_core.h"

namespace {

// ---- vs_png_filter -------------------------------------------------------------------------------------------------------------------
constexpr int FLT_WAVES = 4;                  // rows per workgroup

// bytes p[j .. j + 4) of a row as one little-endian word; a byte at a negative position, or of a null row, reads as zero.  `aligned`:
// p + j is a multiple of 4 (uniform over the wave); j + 4 <= the row's bytes
__device__ __forceinline__ uint32_t row_word(const uint8_t* p, int j, bool aligned) {
    if (p == nullptr) return 0u;
    if (aligned && j >= 0) return *reinterpret_cast<const uint32_t*>(__builtin_assume_aligned(p + j, 4));
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (j + k >= 0) w |= (uint32_t)p[j + k] << (8 * k);
    return w;
}
__device__ __forceinline__ int row_byte(const uint8_t* p, int j) { return (p != nullptr && j >= 0) ? p[j] : 0; }

// The four bytes at j .. j + 3 of a row with their left, above and above-left neighbours, each as one word
struct Quad {
    uint32_t x, a, b, c;
    __device__ __forceinline__ Quad(const uint8_t* cur, const uint8_t* up, int j, int C, bool cur_aligned, bool up_aligned) {
        const int sh = 8 * (4 - C);
        x = row_word(cur, j, cur_aligned);
        b = row_word(up, j, up_aligned);
        a = (uint32_t)((((uint64_t)x << 32) | row_word(cur, j - 4, cur_aligned)) >> sh);
        c = (uint32_t)((((uint64_t)b << 32) | row_word(up, j - 4, up_aligned)) >> sh);
    }
};

__global__ __launch_bounds__(64 * FLT_WAVES) void png_filter_kernel(const uint8_t* __restrict__ pixels, int64_t rows, int H, int row_bytes, int C,
                                                                    int mode, uint8_t* __restrict__ raw, int64_t raw_stride) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * FLT_WAVES + (threadIdx.x >> 6);
    if (r >= rows) return;                    // (no barrier in this kernel: a wave may leave)
    const int64_t img = r / H;
    const int y = (int)(r - img * H);
    const uint8_t* cur = pixels + r * row_bytes;
    const uint8_t* up = y > 0 ? cur - row_bytes : nullptr;                  // the row above row 0 of every image is zeros
    uint8_t* out = raw + img * raw_stride + (int64_t)y * (row_bytes + 1);
    int f = mode;
    if (mode == VPE_MODE_ADAPTIVE) {
        uint32_t sums[5] = {0u, 0u, 0u, 0u, 0u};
        int head = (int)((4 - ((uintptr_t)cur & 3)) & 3);
        if (head > row_bytes) head = row_bytes;
        const int words = (row_bytes - head) >> 2;
        const bool up_aligned = (((uintptr_t)cur - (uintptr_t)row_bytes + (uintptr_t)head) & 3) == 0;
        for (int w = lane; w < words; w += 64) {
            const Quad q(cur, up, head + 4 * w, C, true, up_aligned);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                vpe_add_costs(sums, (q.x >> (8 * k)) & 255, (q.a >> (8 * k)) & 255, (q.b >> (8 * k)) & 255, (q.c >> (8 * k)) & 255);
        }
        const int rest = row_bytes - 4 * words;                             // head + tail: at most 6 bytes
        if (lane < rest) {
            const int j = lane < head ? lane : 4 * words + lane;
            vpe_add_costs(sums, cur[j], row_byte(cur, j - C), row_byte(up, j), row_byte(up, j - C));
        }
#pragma unroll
        for (int t = 0; t < 5; ++t) sums[t] = wave_sum(sums[t]);            // below 65536 * 128
        f = vpe_choose(sums);
    }
    uint8_t* dst = out + 1;
    int head = (int)((4 - ((uintptr_t)dst & 3)) & 3);
    if (head > row_bytes) head = row_bytes;
    const int words = (row_bytes - head) >> 2;
    const bool cur_aligned = (((uintptr_t)cur + (uintptr_t)head) & 3) == 0;
    const bool up_aligned = (((uintptr_t)cur - (uintptr_t)row_bytes + (uintptr_t)head) & 3) == 0;
    for (int w = lane; w < words; w += 64) {
        const int j = head + 4 * w;
        const Quad q(cur, up, j, C, cur_aligned, up_aligned);
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            v |= vpe_residual(f, (q.x >> (8 * k)) & 255, (q.a >> (8 * k)) & 255, (q.b >> (8 * k)) & 255, (q.c >> (8 * k)) & 255) << (8 * k);
        *reinterpret_cast<uint32_t*>(__builtin_assume_aligned(dst + j, 4)) = v;
    }
    const int rest = row_bytes - 4 * words;
    if (lane < rest) {
        const int j = lane < head ? lane : 4 * words + lane;
        dst[j] = (uint8_t)vpe_residual(f, cur[j], row_byte(cur, j - C), row_byte(up, j), row_byte(up, j - C));
    }
    if (lane == 0) out[0] = (uint8_t)f;
}

// ---- vs_deflate_streams --------------------------------------------------------------------------------------------------------------
constexpr int STAGE_BYTES = VSD_MAX_CHUNK + 16;
constexpr int IMAGE_WORDS = (VSD_MAX_CHUNK + VSD_SLOT_EXTRA + 3) / 4;
// the window kernel: the image shares its bytes with the history, which is dead when the image is first written (vs_deflate.hip)
constexpr int WIN_X_AT = 48 + VSW_MAX_HISTORY;
constexpr int WIN_STAGE_BYTES = WIN_X_AT + 16 + VSD_MAX_CHUNK;
static_assert(WIN_X_AT % 16 == 0 && (IMAGE_WORDS + 3) / 4 * 16 <= WIN_X_AT, "the image ends before the chunk");
static_assert(VS_DEFLATE_WINDOW_GROUP_BYTES == 4 * VSD_MAX_CHUNK, "one word per position of a chunk");

// g[0 .. total) into y[0 .. total), which share their offset inside a 16-byte line: 16-byte lines, head and tail by bytes
__device__ __forceinline__ void stage_lines(uint8_t* y, const uint8_t* g, int total, int lane) {
    int head = (int)((16 - ((uintptr_t)g & 15)) & 15);
    if (head > total) head = total;
    const int vecs = (total - head) >> 4;
    if (lane < head) y[lane] = g[lane];
    for (int v = lane; v < vecs; v += 64) *reinterpret_cast<u32x4*>(y + head + 16 * v) = *reinterpret_cast<const u32x4*>(g + head + 16 * v);
    for (int i = head + 16 * vecs + lane; i < total; i += 64) y[i] = g[i];   // at most 15 bytes
}
// size bytes of the image into the slot: 16-byte stores when the slot is aligned so, bytes otherwise
__device__ __forceinline__ void store_slot(uint8_t* slot, const uint8_t* img, int size, int lane) {
    int done = 0;
    if (((uintptr_t)slot & 15) == 0) {
        const int full = size >> 4;
        for (int v = lane; v < full; v += 64) reinterpret_cast<u32x4*>(slot)[v] = reinterpret_cast<const u32x4*>(img)[v];
        done = full << 4;
    }
    for (int i = done + lane; i < size; i += 64) slot[i] = img[i];
}

__global__ __launch_bounds__(64) void deflate_streams_kernel(const uint8_t* __restrict__ src, int64_t stream_bytes, int64_t stream_stride,
                                                             int chunk_bytes, int64_t K, uint8_t* __restrict__ slots, int64_t slot_stride,
                                                             int64_t* __restrict__ sizes) {
    __shared__ VsdWork work;
    __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE_BYTES];
    __shared__ __attribute__((aligned(16))) uint32_t image[(IMAGE_WORDS + 3) / 4 * 4];
    const int lane = threadIdx.x;
    const int64_t c = blockIdx.x, s = c / K;
    int64_t lo;
    int n, hist;
    vpe_chunk(stream_bytes, chunk_bytes, c - s * K, &lo, &n, &hist);
    const uint8_t* in = src + s * stream_stride + lo;
    uint8_t* x = stage + (int)((uintptr_t)in & 15);                         // x + i and in + i share their offset inside a 16-byte line
    stage_lines(x, in, n, lane);
    const int size = vsd_deflate_chunk(x, n, &work, image, lane, 64);
    store_slot(slots + c * slot_stride, reinterpret_cast<const uint8_t*>(image), size, lane);
    if (lane == 0) sizes[c] = size;
}

// One workgroup of one wave loops over the chunks c = blockIdx.x, blockIdx.x + gridDim.x, ... of all streams; its per-position words are
// its own VS_DEFLATE_WINDOW_GROUP_BYTES of the workspace.
__global__ __launch_bounds__(64) void deflate_streams_window_kernel(const uint8_t* __restrict__ src, int64_t stream_bytes, int64_t stream_stride,
                                                                    int chunk_bytes, int64_t K, int64_t chunks, uint8_t* __restrict__ slots,
                                                                    int64_t slot_stride, int64_t* __restrict__ sizes, uint32_t* __restrict__ workspace) {
    __shared__ VsdWork runs_work;
    __shared__ VsdWork window_work;
    __shared__ VswWork search;
    __shared__ __attribute__((aligned(16))) uint8_t stage[WIN_STAGE_BYTES];
    const int lane = threadIdx.x;
    uint32_t* pk = workspace + (int64_t)blockIdx.x * VSD_MAX_CHUNK;
    uint32_t* image = reinterpret_cast<uint32_t*>(stage);
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t s = c / K;
        int64_t lo;
        int n, hist;
        vpe_chunk(stream_bytes, chunk_bytes, c - s * K, &lo, &n, &hist);    // hist <= lo: never before the stream's first byte
        const uint8_t* in = src + s * stream_stride + lo;
        uint8_t* x = stage + WIN_X_AT + (int)((uintptr_t)in & 15);          // x + i and in + i share their offset inside a 16-byte line
        __syncthreads();                                                    // the previous chunk's image has left the stage
        stage_lines(x - hist, in - hist, hist + n, lane);                   // x - hist >= stage + 48
        const int size = vsw_deflate_chunk(x, hist, n, &runs_work, &window_work, &search, pk, image, lane, 64);
        store_slot(slots + c * slot_stride, stage, size, lane);
        if (lane == 0) sizes[c] = size;
    }
}

// ---- vs_png_assemble -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ASM_THREADS) void png_assemble_kernel(const uint8_t* __restrict__ raw, int64_t raw_stride, int64_t S,
                                                                   const uint8_t* __restrict__ slots, int64_t slot_stride,
                                                                   const int64_t* __restrict__ sizes, int64_t K, const VpeLead lead, uint8_t* files,
                                                                   int64_t file_stride, int64_t* __restrict__ file_bytes) {
    __shared__ uint32_t table[256];
    table[threadIdx.x] = vsd_crc_table_entry(threadIdx.x);                  // 256 threads, 256 entries
    __syncthreads();
    const int64_t i = blockIdx.x;
    const int64_t bytes = vpe_assemble(files + i * file_stride, file_stride, lead, slots + i * K * slot_stride, slot_stride, sizes + i * K, K,
                                       raw + i * raw_stride, S, table, threadIdx.x, ASM_THREADS);
    if (threadIdx.x == 0) file_bytes[i] = bytes;
}
static_assert(ASM_THREADS == 256, "one thread per entry of the CRC table");

}  // namespace

extern "C" int vs_png_filter(const uint8_t* pixels, int64_t n, int H, int W, int C, int mode, uint8_t* raw, int64_t raw_stride, void* stream) {
    VS_CHECK_ARG(pixels && raw, "vs_png_filter: null pointer");
    VS_CHECK_ARG(n > 0 && H > 0 && W > 0, "vs_png_filter: sizes must be positive (n %lld, image %d x %d)", (long long)n, H, W);
    VS_CHECK_ARG(C >= 1 && C <= 4, "vs_png_filter: 1..4 channels (got %d)", C);
    VS_CHECK_ARG(mode >= 0 && mode <= VPE_MODE_ADAPTIVE, "vs_png_filter: mode %d outside 0 .. 5 (a filter type, or 5 for adaptive)", mode);
    VS_CHECK_ARG(1 + (int64_t)W * C <= 65536, "vs_png_filter: a row of %lld bytes exceeds 65536", 1 + (long long)W * C);
    VS_CHECK_ARG(raw_stride >= (int64_t)H * (1 + (int64_t)W * C), "vs_png_filter: raw_stride %lld is less than the %d rows of %lld bytes",
                 (long long)raw_stride, H, 1 + (long long)W * C);
    const int64_t rows = n * H, blocks = (rows + FLT_WAVES - 1) / FLT_WAVES;
    VS_CHECK_ARG(n <= 2147483647ll && blocks <= 2147483647ll, "vs_png_filter: %lld rows exceed the grid limit", (long long)rows);
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)blocks), dim3(64 * FLT_WAVES), 0, (hipStream_t)stream, pixels, rows, H, W * C, C, mode, raw,
                       raw_stride);
    VS_CHECK_LAUNCH("vs_png_filter");
    return VS_OK;
}

extern "C" int vs_deflate_streams(const uint8_t* src, int64_t n_streams, int64_t stream_bytes, int64_t stream_stride, int chunk_bytes, int match,
                                  uint8_t* slots, int64_t slot_stride, int64_t* sizes, void* workspace, int64_t workspace_bytes, void* stream) {
    VS_CHECK_ARG(src && slots && sizes, "vs_deflate_streams: null pointer");
    VS_CHECK_ARG(n_streams > 0 && stream_bytes > 0, "vs_deflate_streams: sizes must be positive (%lld streams of %lld bytes)", (long long)n_streams,
                 (long long)stream_bytes);
    VS_CHECK_ARG(stream_stride >= stream_bytes, "vs_deflate_streams: stream_stride %lld is less than the %lld bytes of a stream",
                 (long long)stream_stride, (long long)stream_bytes);
    VS_CHECK_ARG(match == 0 || match == 1, "vs_deflate_streams: match %d: 0 (runs) or 1 (window) expected", match);
    VS_CHECK_ARG(chunk_bytes >= VS_DEFLATE_MIN_CHUNK && chunk_bytes <= VS_DEFLATE_MAX_CHUNK, "vs_deflate_streams: chunk_bytes %d outside %d .. %d",
                 chunk_bytes, VS_DEFLATE_MIN_CHUNK, VS_DEFLATE_MAX_CHUNK);
    VS_CHECK_ARG(slot_stride >= (int64_t)chunk_bytes + VS_DEFLATE_SLOT_EXTRA, "vs_deflate_streams: slot_stride %lld is below the worst case %d + %d",
                 (long long)slot_stride, chunk_bytes, VS_DEFLATE_SLOT_EXTRA);
    const int64_t K = vpe_chunks_per_stream(stream_bytes, chunk_bytes);
    VS_CHECK_ARG(n_streams <= 2147483647ll / K, "vs_deflate_streams: %lld streams of %lld chunks exceed the grid limit", (long long)n_streams,
                 (long long)K);
    const int64_t chunks = n_streams * K;
    if (match == 0) {
        hipLaunchKernelGGL(deflate_streams_kernel, dim3((unsigned)chunks), dim3(64), 0, (hipStream_t)stream, src, stream_bytes, stream_stride,
                           chunk_bytes, K, slots, slot_stride, sizes);
    } else {
        VS_CHECK_ARG(workspace && ((uintptr_t)workspace & 3) == 0 && workspace_bytes >= VS_DEFLATE_WINDOW_GROUP_BYTES,
                     "vs_deflate_streams: workspace %p of %lld bytes; %d bytes per workgroup at a 4-byte boundary are needed", workspace,
                     (long long)workspace_bytes, VS_DEFLATE_WINDOW_GROUP_BYTES);
        int64_t groups = workspace_bytes / VS_DEFLATE_WINDOW_GROUP_BYTES;
        if (groups > chunks) groups = chunks;
        hipLaunchKernelGGL(deflate_streams_window_kernel, dim3((unsigned)groups), dim3(64), 0, (hipStream_t)stream, src, stream_bytes, stream_stride,
                           chunk_bytes, K, chunks, slots, slot_stride, sizes, (uint32_t*)workspace);
    }
    VS_CHECK_LAUNCH("vs_deflate_streams");
    return VS_OK;
}

extern "C" int vs_png_assemble(const uint8_t* raw, int64_t raw_stride, const uint8_t* slots, int64_t slot_stride, const int64_t* sizes, int64_t n,
                               int H, int W, int C, int64_t chunks_per_image, uint8_t* files, int64_t file_stride, int64_t* file_bytes, void* stream) {
    VS_CHECK_ARG(raw && slots && sizes && files && file_bytes, "vs_png_assemble: null pointer");
    VS_CHECK_ARG(n > 0 && H > 0 && W > 0 && chunks_per_image > 0 && slot_stride > 0,
                 "vs_png_assemble: sizes must be positive (n %lld, image %d x %d, %lld chunks per image, slot_stride %lld)", (long long)n, H, W,
                 (long long)chunks_per_image, (long long)slot_stride);
    VS_CHECK_ARG(C >= 1 && C <= 4, "vs_png_assemble: 1..4 channels (got %d)", C);
    const int64_t S = (int64_t)H * (1 + (int64_t)W * C), K = chunks_per_image;
    VS_CHECK_ARG(raw_stride >= S, "vs_png_assemble: raw_stride %lld is less than the %d rows of %lld bytes", (long long)raw_stride, H,
                 1 + (long long)W * C);
    VS_CHECK_ARG(K <= S, "vs_png_assemble: %lld chunks for %lld bytes", (long long)K, (long long)S);
    VS_CHECK_ARG(S + VS_DEFLATE_SLOT_EXTRA * K + 8 < (1ll << 31), "vs_png_assemble: an IDAT body of up to %lld bytes does not fit one chunk (2^31)",
                 (long long)(S + VS_DEFLATE_SLOT_EXTRA * K + 8));
    VS_CHECK_ARG(file_stride >= vpe_file_bound(S, K), "vs_png_assemble: file_stride %lld is below the worst case 57 + 8 + %lld + %d * %lld",
                 (long long)file_stride, (long long)S, VS_DEFLATE_SLOT_EXTRA, (long long)K);
    VS_CHECK_ARG(n <= 2147483647ll, "vs_png_assemble: %lld images exceed the grid limit", (long long)n);
    hipLaunchKernelGGL(png_assemble_kernel, dim3((unsigned)n), dim3(ASM_THREADS), 0, (hipStream_t)stream, raw, raw_stride, S, slots, slot_stride, sizes, K,
                       vpe_lead(W, H, C), files, file_stride, file_bytes);
    VS_CHECK_LAUNCH("vs_png_assemble");
    return VS_OK;
}

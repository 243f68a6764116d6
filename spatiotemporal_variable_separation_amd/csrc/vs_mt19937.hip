// vs_mt19937.hip -- NumPy's legacy random stream on the device: vs_mt19937_randint draws a table of scalar `randint(low, high)` values from
// an MT19937 state that lives in HBM, bit for bit what np.random.RandomState gives for the same calls in the same order.  The Moving-MNIST
// training loader draws its five integers per digit with it (data/numpy_stream.py), so that no draw, upload or synchronisation is left on
// the host per batch.
//
// The logic (regeneration, tempering, masked rejection, which draw takes which output) is csrc/vs_mt19937_core.h, which also runs on the
// CPU; this file adds the lane primitives.  A stream is one sequence, so one launch is ONE WORKGROUP of four waves and launches on one
// stream are serialised by their order.  Per launch, in LDS (5 KiB): the block and the block being made (2 x 624 words) and the waves'
// partial scans.  A window of 256 outputs is tempered at once; the packed maps are scanned inside each wave with __shfl_up (6 steps) and
// the four waves' totals are combined through LDS, likewise the counts of accepted outputs.
#include "vs_common.h"

namespace {

constexpr int MT_WAVES = 4;

__device__ inline uint32_t mt_compose(uint32_t a, uint32_t b);

__device__ __forceinline__ void block_scan_map(uint32_t m, uint32_t& before, uint32_t& total) {
    __shared__ uint32_t wave_total[MT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = m;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t lower = (uint32_t)__shfl_up((int)incl, o, 64);
        if (lane >= o) incl = mt_compose(lower, incl);
    }
    uint32_t excl = (uint32_t)__shfl_up((int)incl, 1, 64);
    if (lane == 0) excl = 0x76543210u;
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();                                // the next write of wave_total lies behind the barriers of the add scan and the window's end
    uint32_t pre = 0x76543210u, all = 0x76543210u;
#pragma unroll
    for (int wv = 0; wv < MT_WAVES; ++wv) {
        if (wv == wave) pre = all;
        all = mt_compose(all, wave_total[wv]);
    }
    before = mt_compose(pre, excl);
    total = all;
}

__device__ __forceinline__ void block_scan_add(int v, int& before, int& total) {
    __shared__ int wave_total[MT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int lower = __shfl_up(incl, o, 64);
        if (lane >= o) incl += lower;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();                                // the next write lies behind the barriers of the window's end and of the next map scan
    int pre = 0, all = 0;
#pragma unroll
    for (int wv = 0; wv < MT_WAVES; ++wv) {
        if (wv == wave) pre = all;
        all += wave_total[wv];
    }
    before = pre + incl - v;
    total = all;
}

}  // namespace

// the workgroup's forms of the core's primitives (the core is compiled for the device only here)
#define VSM_HD __device__ inline
#define VSM_SYNC() __syncthreads()
#define VSM_SCAN_MAP(m, before, total) block_scan_map((m), (before), (total))
#define VSM_SCAN_ADD(v, before, total) block_scan_add((v), (before), (total))
#include "vs_mt19937_core.h"

namespace {

__device__ inline uint32_t mt_compose(uint32_t a, uint32_t b) { return vsm_compose(a, b); }

__global__ __launch_bounds__(64 * MT_WAVES) void mt19937_randint_kernel(uint32_t* __restrict__ state, VsmCols cols, int64_t n_rows,
                                                                        int32_t* __restrict__ out, int32_t* __restrict__ bad) {
    __shared__ VsmWork work;
    const int status = vsm_fill_table(state, &work, &cols, n_rows, out, (int)threadIdx.x, 64 * MT_WAVES);
    if (status != VSM_STATUS_OK && bad != nullptr && threadIdx.x == 0) *bad = status;
}

}  // namespace

extern "C" int vs_mt19937_randint(uint32_t* state, const int32_t* lows, const int32_t* highs, int k, int64_t n_rows, int32_t* out, int32_t* bad,
                                  void* stream) {
    VS_CHECK_ARG(state && lows && highs && out, "vs_mt19937_randint: null pointer");
    VS_CHECK_ARG(k >= 1 && k <= VS_MT19937_MAX_COLS, "vs_mt19937_randint: k %d outside 1 .. %d", k, VS_MT19937_MAX_COLS);
    VS_CHECK_ARG(n_rows >= 0 && n_rows <= VS_MT19937_MAX_ROWS, "vs_mt19937_randint: n_rows %lld outside 0 .. 2^40", (long long)n_rows);
    for (int j = 0; j < k; ++j)
        VS_CHECK_ARG(lows[j] < highs[j], "vs_mt19937_randint: column %d has low %d >= high %d", j, lows[j], highs[j]);
    if (n_rows == 0) return VS_OK;
    VsmCols cols;
    vsm_cols_init(&cols, lows, highs, k);
    hipLaunchKernelGGL(mt19937_randint_kernel, dim3(1), dim3(64 * MT_WAVES), 0, (hipStream_t)stream, state, cols, n_rows, out, bad);
    VS_CHECK_LAUNCH("vs_mt19937_randint");
    return VS_OK;
}

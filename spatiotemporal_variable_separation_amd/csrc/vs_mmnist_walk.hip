// vs_mmnist_walk.hip -- the stochastic Moving-MNIST trajectories on the device: vs_mmnist_stochastic_trajectories walks a batch of
// trajectories of the reference's sampler with deterministic=False (data/moving_mnist.py:131-253), which redraws the speed from the NumPy
// stream at every bounce, from an MT19937 state that lives in HBM (data/numpy_stream.py), bit for bit what the reference's Python gives
// for the same stream.  The host route is a Python loop of some tens of microseconds per trajectory; this is one launch per batch.
//
// The logic is csrc/vs_mmnist_walk_core.h (which also runs on the CPU) on top of csrc/vs_mt19937_core.h; this file adds the barrier.  The
// stream is one sequence, so one launch is ONE WORKGROUP and launches on one HIP stream continue the sequence in their order.  The lanes
// form of the core runs: a window of four blocks in LDS (10 KiB), every lane walks trajectories from the window's offsets without storing
// them (2 to 3 offsets per lane and round at 1024 lanes), the true starts are chased through the table of ends by pointer doubling (two
// uint16 tables, 10 KiB), the lanes of the true starts walk again and store.  The walk is double arithmetic (the reference's Python
// floats) with contraction off.
#include "vs_common.h"

// the workgroup's forms of the cores' primitives (the cores are compiled for the device only here; the scans belong to vsm_fill_table,
// which this file does not call)
#define VSM_HD __device__ inline
#define VSM_SYNC() __syncthreads()
#define VSM_SCAN_MAP(m, before, total) ((before) = VSM_IDENTITY, (total) = (m))
#define VSM_SCAN_ADD(v, before, total) ((before) = 0, (total) = (v))
#include "vs_mmnist_walk_core.h"

namespace {

constexpr int WALK_LANES = 1024;

__global__ __launch_bounds__(WALK_LANES) void mmnist_walk_kernel(uint32_t* __restrict__ state, VswGeom geom, int64_t n_traj,
                                                                 const int32_t* __restrict__ start, int32_t* __restrict__ pre,
                                                                 int32_t* __restrict__ positions, int32_t* __restrict__ latents,
                                                                 int32_t* __restrict__ desc, int nd, int32_t* __restrict__ bad) {
    __shared__ VswWork work;
    const int status = vsw_walk_lanes(state, &work, &geom, n_traj, start, pre, positions, latents, desc, nd, (int)threadIdx.x, WALK_LANES);
    if (status != VSM_STATUS_OK && bad != nullptr && threadIdx.x == 0) *bad = status;
}

}  // namespace

extern "C" int vs_mmnist_stochastic_trajectories(uint32_t* state, const int32_t* lows, const int32_t* highs, int n_pre, int64_t n_traj, int seq_len,
                                                 int x_max, int y_max, int max_speed, const int32_t* start, int32_t* pre, int32_t* positions,
                                                 int32_t* latents, int32_t* desc, int desc_nd, int32_t* bad, void* stream) {
    const char* me = "vs_mmnist_stochastic_trajectories";
    VS_CHECK_ARG(state && positions, "%s: null pointer (state, positions)", me);
    VS_CHECK_ARG(n_pre >= 0 && n_pre <= VS_MMNIST_WALK_MAX_PRE, "%s: n_pre %d outside 0 .. %d", me, n_pre, VS_MMNIST_WALK_MAX_PRE);
    VS_CHECK_ARG(n_pre == 0 || (lows && highs && pre), "%s: null pointer (lows, highs, pre with n_pre %d)", me, n_pre);
    VS_CHECK_ARG(n_pre >= 4 || start, "%s: null pointer (n_pre %d needs the start table)", me, n_pre);
    VS_CHECK_ARG(seq_len >= 1 && seq_len <= (1 << 20), "%s: seq_len %d outside 1 .. 2^20", me, seq_len);
    VS_CHECK_ARG(n_traj >= 0 && n_traj <= VS_MMNIST_WALK_MAX_TRAJ, "%s: n_traj %lld outside 0 .. 2^24", me, (long long)n_traj);
    VS_CHECK_ARG(x_max >= 1 && y_max >= 1, "%s: x_max %d, y_max %d: both must be >= 1 (a digit that fills the frame is unsupported)", me, x_max,
                 y_max);
    VS_CHECK_ARG(max_speed >= 0 && max_speed <= (1 << 20), "%s: max_speed %d outside 0 .. 2^20", me, max_speed);
    for (int j = 0; j < n_pre; ++j) VS_CHECK_ARG(lows[j] < highs[j], "%s: column %d has low %d >= high %d", me, j, lows[j], highs[j]);
    if (desc)
        VS_CHECK_ARG(n_pre == 5 && desc_nd >= 1 && desc_nd <= 8 && n_traj % desc_nd == 0,
                     "%s: desc needs n_pre 5 and 1 .. 8 digits per video that divide n_traj (n_pre %d, nd %d, n_traj %lld)", me, n_pre, desc_nd,
                     (long long)n_traj);
    if (n_traj == 0) return VS_OK;
    VswGeom geom;
    vsw_geom_init(&geom, n_pre, seq_len, lows, highs, x_max, y_max, max_speed);
    hipLaunchKernelGGL(mmnist_walk_kernel, dim3(1), dim3(WALK_LANES), 0, (hipStream_t)stream, state, geom, n_traj, start, pre, positions, latents,
                       desc, desc ? desc_nd : 1, bad);
    VS_CHECK_LAUNCH(me);
    return VS_OK;
}

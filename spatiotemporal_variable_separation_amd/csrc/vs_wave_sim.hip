// vs_wave_sim.hip -- the WaveEq data set simulated on the device (reference: preprocessing/wave/gen_wave.py:37-92 `derivative` and
// :121-135, the body of `generate`).
//
// The reference integrates, per sequence, the state y = (w, w') (two fp32 [64, 64] fields, zero at the start) of
//     y' = f(t, y) = (w',  c^2 * (w_yy + w_xx) + s(t) * mask)
// with torchdiffeq.odeint(method="rk4") on the grid t = arange(0, dt * T, dt) (fp32), one step per grid interval, h = t[i+1] - t[i]:
//   * w_yy[:, i] = -1/12 w[:, i+2] + 4/3 w[:, i+1] - 5/2 w[:, i] + 4/3 w[:, i-1] - 1/12 w[:, i-2] for i in 2..61 and ZERO in columns
//     0, 1, 62, 63; w_xx[j, :] is the same stencil along the first axis for j in 2..61 and ZERO in rows 0, 1, 62, 63.  The two border
//     bands are per axis: a cell of row 0 and column 10 still gets its w_yy term.  The terms are summed left to right as written;
//   * mask = (col - 32)^2 + (row - 32)^2 < 25, s(t) = f0 * exp(-20 t), c^2 rounded to fp32 once, dx = 1;
//   * torchdiffeq's fixed-grid "rk4" is the 3/8 rule (`rk4_alt_step_func`), NOT the classical tableau:
//         k1 = f(t0, y)
//         k2 = f(t0 + h/3,  y + h k1 / 3)                  computed as  y + (h * k1) * (1/3)
//         k3 = f(t0 + 2h/3, y + h (k2 - k1 / 3))           computed as  y + h * (k2 - k1 * (1/3))
//         k4 = f(t1,        y + h (k1 - k2 + k3))
//         y += (k1 + 3 (k2 + k3) + k4) h / 8               computed as  ((k1 + 3 * (k2 + k3)) + k4) * h * 0.125
//     (stated from knowledge of torchdiffeq 0.2; the package is no dependency of this project: a reader who has it can compare);
//   * frame i of the output is w after i steps, frame 0 is the initial w.
//
// The source term never sees an exp on the device: the caller tabulates s at the 3 (T - 1) + 1 stage times of a sequence the way the
// reference rounds it (times formed in fp32, widened, f0 * exp(-20 t) in fp64, rounded to fp32) and the kernel reads src[3 i + stage];
// stage 4 of step i is stage 1 of step i + 1 (t1 = t[i+1]).  The step sizes h come as a table too, they are differences of fp32 grid times.
//
// Kernel: one workgroup of 256 threads carries one sequence from the first frame to the last.  Thread (ty, tx) of a 16 x 16 arrangement
// owns the 4 x 4 cells at rows 4 ty.., columns 4 tx.. and keeps w, w' and the stage derivatives of those cells in registers for the
// whole simulation.  Per stage the threads publish the stage's w to an LDS image (a 2-row / 4-column border of cells that nobody
// writes, so that every neighbour read stays inside the image; what is read there is discarded by the border rule), meet at ONE
// barrier, and read the 32 neighbour cells around their block (16 B and 8 B LDS reads); their own 16 cells never leave the registers.
// Two images alternate: a stage's image is overwritten two barriers later, when every thread has consumed it.  That is 4 barriers per
// step; HBM is touched only to write a frame per step (one 16 B store per thread and row: 256 B contiguous per row).
// Two workgroups fit a CU (launch bound: two waves per SIMD, 256 registers a thread, 2 x 43.5 KB of LDS), so the 300 sequences of the
// paper's set are one round on 256 CUs.
// The running minimum and maximum of w over all frames ride along in registers; with `normalise` every thread finally rewrites ITS OWN stores as
// (x - min) / (max - min) with an IEEE division, the arithmetic of the file loader (data/wave_eq.py).
#include "vs_common.h"

namespace {

constexpr int WN = 64;                  // frame edge (the reference's mask is hard-coded to this grid)
constexpr int WPITCH = 80;              // 4 + 64 + 4 columns, padded so that 4 rows apart is a multiple of 64 banks (16 B reads of two
                                        // thread rows then fall on disjoint banks)
constexpr int WROWS = WN + 4;           // 2 + 64 + 2 rows
constexpr int WIMG = WROWS * WPITCH;

struct Cells { float a[4][4]; };

// c^2 (w_yy + w_xx) + s mask of the thread's 16 cells for the stage field `sw`, published to `img` first
__device__ __forceinline__ void wave_accel(const Cells& sw, float* __restrict__ img, int r0, int c0, float c2, float s, unsigned disc, Cells& out) {
    const float A = (float)(-1.0 / 12.0), B = (float)(4.0 / 3.0), D = (float)(5.0 / 2.0), E = (float)(1.0 / 12.0);
    float* base = img + (r0 + 2) * WPITCH + c0 + 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const f32x4 q = {sw.a[r][0], sw.a[r][1], sw.a[r][2], sw.a[r][3]};
        *reinterpret_cast<f32x4*>(base + r * WPITCH) = q;
    }
    __syncthreads();
    float row[4][8], col[8][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const f32x2 l = *reinterpret_cast<const f32x2*>(base + r * WPITCH - 2);
        const f32x2 g = *reinterpret_cast<const f32x2*>(base + r * WPITCH + 4);
        row[r][0] = l[0]; row[r][1] = l[1]; row[r][6] = g[0]; row[r][7] = g[1];
#pragma unroll
        for (int j = 0; j < 4; ++j) { row[r][j + 2] = sw.a[r][j]; col[r + 2][j] = sw.a[r][j]; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int rr = k < 2 ? k - 2 : k + 2;              // rows -2, -1, 4, 5 of the block
        const f32x4 q = *reinterpret_cast<const f32x4*>(base + rr * WPITCH);
#pragma unroll
        for (int j = 0; j < 4; ++j) col[rr + 2][j] = q[j];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const bool row_in = (unsigned)(r0 + r - 2) < (unsigned)(WN - 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool col_in = (unsigned)(c0 + j - 2) < (unsigned)(WN - 4);
            float yy = A * row[r][j + 4] + B * row[r][j + 3] - D * row[r][j + 2] + B * row[r][j + 1] - E * row[r][j];
            float xx = A * col[r + 4][j] + B * col[r + 3][j] - D * col[r + 2][j] + B * col[r + 1][j] - E * col[r][j];
            yy = col_in ? yy : 0.f;
            xx = row_in ? xx : 0.f;
            const float m = (disc >> (r * 4 + j)) & 1u ? 1.f : 0.f;
            out.a[r][j] = s * m + c2 * (yy + xx);
        }
    }
}

__global__ __launch_bounds__(256, 2) void wave_sim_kernel(const float* __restrict__ c2s, const float* __restrict__ src, const float* __restrict__ hs,
                                                       const float* __restrict__ init, float* out, float* minmax, int T, int normalise) {
    __shared__ __attribute__((aligned(16))) float img[2 * WIMG];
    const int tid = threadIdx.x;
    const int64_t seq = blockIdx.x;
    const int r0 = 4 * (tid >> 4), c0 = 4 * (tid & 15);
    for (int i = tid; i < 2 * WIMG; i += 256) img[i] = 0.f;
    __syncthreads();

    const float c2 = c2s[seq];
    const float* s_tab = src + seq * (3 * (int64_t)(T - 1) + 1);
    const float third = (float)(1.0 / 3.0);
    unsigned disc = 0;
    Cells w, v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int dy = r0 + r - 32, dx = c0 + j - 32;
            if (dx * dx + dy * dy < 25) disc |= 1u << (r * 4 + j);
            w.a[r][j] = 0.f; v.a[r][j] = 0.f;
        }
        if (init) {
            const float* p = init + seq * 2 * WN * WN + (r0 + r) * WN + c0;
            const f32x4 qw = *reinterpret_cast<const f32x4*>(p), qv = *reinterpret_cast<const f32x4*>(p + WN * WN);
#pragma unroll
            for (int j = 0; j < 4; ++j) { w.a[r][j] = qw[j]; v.a[r][j] = qv[j]; }
        }
    }
    float* frame = out + seq * T * WN * WN + r0 * WN + c0;
    float mn = w.a[0][0], mx = w.a[0][0];
    auto emit = [&](int t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const f32x4 q = {w.a[r][0], w.a[r][1], w.a[r][2], w.a[r][3]};
            *reinterpret_cast<f32x4*>(frame + (int64_t)t * WN * WN + r * WN) = q;
#pragma unroll
            for (int j = 0; j < 4; ++j) { mn = fminf(mn, q[j]); mx = fmaxf(mx, q[j]); }
        }
    };
    emit(0);

    for (int i = 0; i + 1 < T; ++i) {
        const float h = hs[i];
        const float s0 = s_tab[3 * i], s1 = s_tab[3 * i + 1], s2 = s_tab[3 * i + 2], s3 = s_tab[3 * i + 3];
        Cells k1v, k2w, k2v, k3w, k3v, k4w, k4v, sw;       // k1w is v itself
        wave_accel(w, img, r0, c0, c2, s0, disc, k1v);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sw.a[r][j] = w.a[r][j] + h * v.a[r][j] * third;
                k2w.a[r][j] = v.a[r][j] + h * k1v.a[r][j] * third;
            }
        wave_accel(sw, img + WIMG, r0, c0, c2, s1, disc, k2v);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sw.a[r][j] = w.a[r][j] + h * (k2w.a[r][j] - v.a[r][j] * third);
                k3w.a[r][j] = v.a[r][j] + h * (k2v.a[r][j] - k1v.a[r][j] * third);
            }
        wave_accel(sw, img, r0, c0, c2, s2, disc, k3v);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sw.a[r][j] = w.a[r][j] + h * (v.a[r][j] - k2w.a[r][j] + k3w.a[r][j]);
                k4w.a[r][j] = v.a[r][j] + h * (k1v.a[r][j] - k2v.a[r][j] + k3v.a[r][j]);
            }
        wave_accel(sw, img + WIMG, r0, c0, c2, s3, disc, k4v);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                w.a[r][j] += (v.a[r][j] + 3.f * (k2w.a[r][j] + k3w.a[r][j]) + k4w.a[r][j]) * h * 0.125f;
                v.a[r][j] += (k1v.a[r][j] + 3.f * (k2v.a[r][j] + k3v.a[r][j]) + k4v.a[r][j]) * h * 0.125f;
            }
        emit(i + 1);
    }

    // minimum and maximum of the workgroup, through the LDS the images used (this barrier: every thread is done reading them)
    __syncthreads();
    img[tid] = mn; img[256 + tid] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { img[tid] = fminf(img[tid], img[tid + s]); img[256 + tid] = fmaxf(img[256 + tid], img[256 + tid + s]); }
        __syncthreads();
    }
    mn = img[0]; mx = img[256];
    if (minmax && tid == 0) { minmax[2 * seq] = mn; minmax[2 * seq + 1] = mx; }
    if (normalise) {                                       // every thread re-reads only what it stored itself
        const float span = mx - mn;
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                f32x4* p = reinterpret_cast<f32x4*>(frame + (int64_t)t * WN * WN + r * WN);
                f32x4 q = *p;
#pragma unroll
                for (int j = 0; j < 4; ++j) q[j] = __fdiv_rn(q[j] - mn, span);
                *p = q;
            }
    }
}

}  // namespace

extern "C" int vs_wave_simulate(int n_seq, int T, int frame_size, const float* c2, const float* source, const float* h, const float* init,
                                float* out, float* minmax, int normalise, void* stream) {
    VS_CHECK_ARG(n_seq >= 1 && T >= 1, "vs_wave_simulate: n_seq and T must be positive (got %d, %d)", n_seq, T);
    VS_CHECK_ARG(frame_size == WN, "vs_wave_simulate: only %dx%d frames (the reference's source disc is fixed to that grid), got %d", WN, WN,
                 frame_size);
    VS_CHECK_ARG(c2 && source && out, "vs_wave_simulate: null pointer");
    VS_CHECK_ARG(h || T == 1, "vs_wave_simulate: the step table is missing");
    VS_CHECK_ARG((uintptr_t)out % 16 == 0 && (uintptr_t)init % 16 == 0, "vs_wave_simulate: out and init must be 16-byte aligned");
    hipLaunchKernelGGL(wave_sim_kernel, dim3((unsigned)n_seq), dim3(256), 0, (hipStream_t)stream, c2, source, h, init, out, minmax, T, normalise);
    VS_CHECK_LAUNCH("vs_wave_simulate");
    return VS_OK;
}

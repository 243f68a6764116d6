// vs_eval.hip -- the device side of the evaluation scripts (reference: test/mnist/test.py, test/mnist/test_disentanglement.py).  The
// content-swap videos are rendered by vs_moving_mnist_place, which lives with the other Moving-MNIST renderers in vs_data.hip.
//
//   * vs_frame_metrics_multi: per-plane MSE and mean SSIM of one prediction against P candidate targets (the best-of-permutations
//     scoring of test_disentanglement.py:153-161).  The window, constants and operation order are those of frame_metrics_kernel
//     (vs_metrics.hip); the prediction plane and its two row-filtered maps stay in LDS across all P targets.
//   * vs_frames_to_u8_nhwc: `x.mul(255).byte().permute(0, 1, 3, 4, 2)` of every saved sample, on the device, so that only uint8 bytes
//     cross PCIe.
//   * vs_sst_frame_metrics: the metrics of test/sst/test.py:57-71, where broadcasting pairs every forecast frame t with the constants of
//     every target day c.  One filter pass over the raw (normalised) planes per frame; the T de-normalised, rescaled variants follow from
//     the window moments by their affine maps, so no [rows, T, T, H, W] tensor exists and 1 plane pair is filtered where the script filters T.
#include "vs_common.h"

namespace {

constexpr int MM_WIN = 11;           // SSIM window (vs_metrics.hip)

struct MmWindow { float g[MM_WIN]; };

// one workgroup per prediction plane; loops over the P targets of that plane.  LDS: the prediction [H][W], one target [H][W], the
// prediction's two row-filtered maps (mu, E[x^2]) [2][H][OW] and the target's three (mu, E[y^2], E[xy]) [3][H][OW] -- the footprint of
// frame_metrics_kernel.  pred [planes] with planes = B * TC; targets [B][P][TC][H][W]; outputs [B][P][TC].
__global__ __launch_bounds__(256) void frame_metrics_multi_kernel(const float* pred, const float* targets, int P, int64_t tc, int H, int W,
                                                                  MmWindow win, float c1, float c2, float* mse, float* ssim) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int64_t plane = blockIdx.x;
    const int64_t b = plane / tc, k = plane - b * tc;
    const int hw = H * W, OW = W - MM_WIN + 1, OH = H - MM_WIN + 1, nh = H * OW, no = OH * OW;
    float* sx = smem;                      // [H][W]
    float* sy = smem + hw;                 // [H][W]
    float* hx = smem + 2 * hw;             // [2][H][OW]: mu_x, E[x^2]
    float* hy = hx + 2 * nh;               // [3][H][OW]: mu_y, E[y^2], E[xy]
    __shared__ float red[2][4];
    const float* px = pred + plane * hw;
    for (int i = threadIdx.x; i < hw; i += 256) sx[i] = px[i];
    __syncthreads();
    for (int i = threadIdx.x; i < nh; i += 256) {
        const int r = i / OW, c = i - r * OW;
        float m1 = 0.f, q1 = 0.f;
#pragma unroll
        for (int j = 0; j < MM_WIN; ++j) {
            const float a = sx[r * W + c + j], g = win.g[j];
            m1 += g * a; q1 += g * (a * a);
        }
        hx[i] = m1; hx[nh + i] = q1;
    }
    for (int p = 0; p < P; ++p) {
        const int64_t o = (b * P + p) * tc + k;
        const float* py = targets + o * hw;
        float se = 0.f;
        for (int i = threadIdx.x; i < hw; i += 256) {
            const float a = sx[i], bb = py[i];
            sy[i] = bb;
            const float d = a - bb;
            se += d * d;
        }
        __syncthreads();                   // sy complete (and, for p = 0, hx); the previous target's readers of hy / red are done
        for (int i = threadIdx.x; i < nh; i += 256) {
            const int r = i / OW, c = i - r * OW;
            float m2 = 0.f, q2 = 0.f, q12 = 0.f;
#pragma unroll
            for (int j = 0; j < MM_WIN; ++j) {
                const float a = sx[r * W + c + j], bb = sy[r * W + c + j], g = win.g[j];
                m2 += g * bb; q2 += g * (bb * bb); q12 += g * (a * bb);
            }
            hy[i] = m2; hy[nh + i] = q2; hy[2 * nh + i] = q12;
        }
        __syncthreads();
        float acc = 0.f;
        for (int i = threadIdx.x; i < no; i += 256) {
            const int r = i / OW, c = i - r * OW;
            float m1 = 0.f, m2 = 0.f, q1 = 0.f, q2 = 0.f, q12 = 0.f;
#pragma unroll
            for (int j = 0; j < MM_WIN; ++j) {
                const int kk = (r + j) * OW + c;
                const float g = win.g[j];
                m1 += g * hx[kk]; m2 += g * hy[kk]; q1 += g * hx[nh + kk]; q2 += g * hy[nh + kk]; q12 += g * hy[2 * nh + kk];
            }
            const float mu1_sq = m1 * m1, mu2_sq = m2 * m2, mu12 = m1 * m2;
            const float v1 = 2.f * (q12 - mu12) + c2, v2 = (q1 - mu1_sq) + (q2 - mu2_sq) + c2;
            acc += ((2.f * mu12 + c1) * v1) / ((mu1_sq + mu2_sq + c1) * v2);
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) { se += __shfl_down(se, s, 64); acc += __shfl_down(acc, s, 64); }
        if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = se; red[1][threadIdx.x >> 6] = acc; }
        __syncthreads();
        if (threadIdx.x == 0) {
            if (mse) mse[o] = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) / (float)hw;
            if (ssim) ssim[o] = no > 0 ? (red[1][0] + red[1][1] + red[1][2] + red[1][3]) / (float)no : 0.f;
        }
        // the next target's first barrier orders these reads of red before its writes
    }
}

__device__ __forceinline__ unsigned int to_u8(float x) {
    const float y = __fmul_rn(x, 255.f);             // one rounded multiply, never contracted
    if (!(y > 0.f)) return 0u;                       // negatives, -0 and NaN
    if (y >= 255.f) return 255u;
    return (unsigned int)y;                          // truncation toward zero, as static_cast<uint8_t>
}

// x [N][C][HW] -> out [N][HW][C]; every thread writes four consecutive output bytes (one 32-bit store when n_out % 4 == 0)
__global__ __launch_bounds__(256) void to_u8_nhwc_kernel(const void* x, int xd, int64_t N, int C, int64_t HW, unsigned char* out) {
    const int64_t n_out = N * C * HW, n4 = (n_out + 3) / 4;
    const int64_t chw = (int64_t)C * HW;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += (int64_t)gridDim.x * 256) {
        unsigned int packed = 0u;
        const int64_t o0 = q * 4;
        const int cnt = n_out - o0 < 4 ? (int)(n_out - o0) : 4;
        for (int e = 0; e < cnt; ++e) {
            const int64_t o = o0 + e;
            const int64_t n = o / chw, rem = o - n * chw;
            const int64_t pix = rem / C, c = rem - pix * C;
            packed |= to_u8(vs_ld(x, xd, n * chw + c * HW + pix)) << (8 * e);
        }
        if (cnt == 4 && (n_out & 3) == 0) {
            reinterpret_cast<unsigned int*>(out)[q] = packed;
        } else {
            for (int e = 0; e < cnt; ++e) out[o0 + e] = (unsigned char)(packed >> (8 * e));
        }
    }
}

constexpr int SM_MAXT = 16;          // target days per window of vs_sst_frame_metrics

// One workgroup per (row, frame t).  LDS as frame_metrics_kernel (vs_metrics.hip): both raw planes and their five row-filtered maps.  The
// script's planes for the constants of day c are x' = a_c x + b_c with a_c = std_norm std_clim / (max - min) and
// b_c = (mu_norm std_clim + mu_clim - min) / (max - min), for forecast and target alike, so per window position
//   mu' = a_c mu + b_c,  var' = a_c^2 var,  cov' = a_c^2 cov
// from the moments of the raw planes; the squared error in original units is (std_norm std_clim)^2 (x - y)^2.  Centred moments are formed
// on the raw z-scored planes (|mu| ~ 1), before the shift b_c, which keeps the cancellation of E[x^2] - mu^2 out of the large offsets.
// A row whose days leave `consts` or whose zone is outside `zone_range` reads no constants, writes zeros and raises *bad.
__global__ __launch_bounds__(256) void sst_frame_metrics_kernel(const float* pred, const float* target, int T, int H, int W, const float* consts,
                                                                int64_t n_days, const int* day0, const int* zone, const float* zone_range,
                                                                int64_t n_zones, MmWindow win, float c1, float c2, float* mse, float* ssim, int* bad) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float sa2[SM_MAXT], sa[SM_MAXT], sb[SM_MAXT], sg2[SM_MAXT];
    __shared__ float red[SM_MAXT + 1][4];
    const int64_t plane = blockIdx.x;                 // row * T + t
    const int64_t row = plane / T;
    const int64_t d0 = day0[row], z = zone[row];
    if (d0 < 0 || d0 + T > n_days || z < 0 || z >= n_zones) {          // uniform over the workgroup
        if (threadIdx.x == 0) {
            if (bad) *bad = 1;
            if (mse) mse[plane] = 0.f;
        }
        if (ssim && (int)threadIdx.x < T) ssim[plane * T + threadIdx.x] = 0.f;
        return;
    }
    if ((int)threadIdx.x < T) {
        const float* k = consts + (d0 + threadIdx.x) * 4;          // mu_norm, std_norm, mu_clim, std_clim
        const float lo = zone_range[z * 2], range = zone_range[z * 2 + 1] - lo;
        const float gain = k[1] * k[3], shift = k[0] * k[3] + k[2];
        const float a = gain / range;
        sa[threadIdx.x] = a; sa2[threadIdx.x] = a * a; sb[threadIdx.x] = (shift - lo) / range; sg2[threadIdx.x] = gain * gain;
    }
    const int hw = H * W, OW = W - MM_WIN + 1, OH = H - MM_WIN + 1, nh = H * OW, no = OH * OW;
    float* sx = smem;                      // [H][W]
    float* sy = smem + hw;                 // [H][W]
    float* hm = smem + 2 * hw;             // [5][H][OW]
    const float* px = pred + plane * hw;
    const float* py = target + plane * hw;
    float se = 0.f;
    for (int i = threadIdx.x; i < hw; i += 256) {
        const float a = px[i], b = py[i];
        sx[i] = a; sy[i] = b;
        const float d = a - b;
        se += d * d;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nh; i += 256) {
        const int r = i / OW, c = i - r * OW;
        float m1 = 0.f, m2 = 0.f, q1 = 0.f, q2 = 0.f, q12 = 0.f;
#pragma unroll
        for (int j = 0; j < MM_WIN; ++j) {
            const float a = sx[r * W + c + j], b = sy[r * W + c + j], g = win.g[j];
            m1 += g * a; m2 += g * b; q1 += g * (a * a); q2 += g * (b * b); q12 += g * (a * b);
        }
        hm[i] = m1; hm[nh + i] = m2; hm[2 * nh + i] = q1; hm[3 * nh + i] = q2; hm[4 * nh + i] = q12;
    }
    __syncthreads();
    float acc[SM_MAXT];
#pragma unroll
    for (int c = 0; c < SM_MAXT; ++c) acc[c] = 0.f;
    for (int i = threadIdx.x; i < no; i += 256) {
        const int r = i / OW, cc = i - r * OW;
        float m1 = 0.f, m2 = 0.f, q1 = 0.f, q2 = 0.f, q12 = 0.f;
#pragma unroll
        for (int j = 0; j < MM_WIN; ++j) {
            const int k = (r + j) * OW + cc;
            const float g = win.g[j];
            m1 += g * hm[k]; m2 += g * hm[nh + k]; q1 += g * hm[2 * nh + k]; q2 += g * hm[3 * nh + k]; q12 += g * hm[4 * nh + k];
        }
        const float var_sum = (q1 - m1 * m1) + (q2 - m2 * m2), cov2 = 2.f * (q12 - m1 * m2);
#pragma unroll
        for (int c = 0; c < SM_MAXT; ++c) {
            if (c < T) {
                const float u1 = sa[c] * m1 + sb[c], u2 = sa[c] * m2 + sb[c];
                const float u12 = u1 * u2, uss = u1 * u1 + u2 * u2;
                acc[c] += ((2.f * u12 + c1) * (sa2[c] * cov2 + c2)) / ((uss + c1) * (sa2[c] * var_sum + c2));
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) se += __shfl_down(se, o, 64);
#pragma unroll
    for (int c = 0; c < SM_MAXT; ++c) {
        if (c < T) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_down(acc[c], o, 64);
        }
    }
    if ((threadIdx.x & 63) == 0) {
        red[SM_MAXT][threadIdx.x >> 6] = se;
#pragma unroll
        for (int c = 0; c < SM_MAXT; ++c) red[c][threadIdx.x >> 6] = acc[c];
    }
    __syncthreads();
    if (ssim && (int)threadIdx.x < T) {
        const int c = threadIdx.x;
        ssim[plane * T + c] = (red[c][0] + red[c][1] + red[c][2] + red[c][3]) / (float)no;
    }
    if (mse && threadIdx.x == 0) {
        float g2 = 0.f;
        for (int c = 0; c < T; ++c) g2 += sg2[c];
        mse[plane] = (red[SM_MAXT][0] + red[SM_MAXT][1] + red[SM_MAXT][2] + red[SM_MAXT][3]) / (float)hw * (g2 / (float)T);
    }
}

}  // namespace

extern "C" int vs_frame_metrics_multi(const float* pred, const float* targets, int64_t batch, int n_targets, int64_t planes_per_sample, int H, int W,
                                      float max_val, float k1, float k2, float sigma, float* mse, float* ssim, void* stream) {
    VS_CHECK_ARG(pred && targets && batch > 0 && n_targets > 0 && planes_per_sample > 0 && batch * planes_per_sample < (1ll << 31) && H >= MM_WIN &&
                     W >= MM_WIN && (mse || ssim),
                 "vs_frame_metrics_multi: bad argument");
    const size_t lds = ((size_t)2 * H * W + (size_t)5 * H * (W - MM_WIN + 1)) * sizeof(float);
    if (lds > 150 * 1024)
        return vs_fail(VS_ERR_UNSUPPORTED, "vs_frame_metrics_multi: planes of %d x %d do not fit the LDS (<= 64 x 64 .. 80 x 80)", H, W);
    MmWindow win;                                    // the window of vs_frame_metrics
    double sum = 0.0, e[MM_WIN];
    for (int j = 0; j < MM_WIN; ++j) {
        const double x = (double)j - (MM_WIN - 1) / 2.0;
        e[j] = exp(-x * x / (2.0 * (double)sigma * (double)sigma));
        sum += e[j];
    }
    for (int j = 0; j < MM_WIN; ++j) win.g[j] = (float)(e[j] / sum);
    const float c1 = (k1 * max_val) * (k1 * max_val), c2 = (k2 * max_val) * (k2 * max_val);
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)frame_metrics_multi_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024) != hipSuccess)
            return vs_fail(VS_ERR_LAUNCH, "vs_frame_metrics_multi: cannot raise the dynamic LDS limit");
        attr_set = true;
    }
    hipLaunchKernelGGL(frame_metrics_multi_kernel, dim3((unsigned)(batch * planes_per_sample)), dim3(256), lds, (hipStream_t)stream, pred, targets,
                       n_targets, planes_per_sample, H, W, win, c1, c2, mse, ssim);
    VS_CHECK_LAUNCH("vs_frame_metrics_multi");
    return VS_OK;
}

extern "C" int vs_frames_to_u8_nhwc(const void* x, int x_dtype, int64_t n, int channels, int64_t hw, uint8_t* out, void* stream) {
    VS_CHECK_ARG(x && out && n > 0 && channels > 0 && hw > 0, "vs_frames_to_u8_nhwc: bad argument");
    VS_CHECK_ARG(vs_dtype_ok(x_dtype), "vs_frames_to_u8_nhwc: bad x_dtype");
    const int64_t n4 = (n * channels * hw + 3) / 4;
    const unsigned blocks = (unsigned)(vs_cdiv(n4, 256) < 2048 ? vs_cdiv(n4, 256) : 2048);
    hipLaunchKernelGGL(to_u8_nhwc_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, x_dtype, n, channels, hw, out);
    VS_CHECK_LAUNCH("vs_frames_to_u8_nhwc");
    return VS_OK;
}

extern "C" int vs_sst_frame_metrics(const float* pred, const float* target, int64_t rows, int T, int H, int W, const float* consts, int64_t n_days,
                                    const int32_t* day0, const int32_t* zone, const float* zone_range, int64_t n_zones, float k1, float k2,
                                    float sigma, float* mse, float* ssim, int32_t* bad, void* stream) {
    VS_CHECK_ARG(pred && target && consts && day0 && zone && zone_range && (mse || ssim), "vs_sst_frame_metrics: null pointer");
    VS_CHECK_ARG(rows > 0 && n_days > 0 && n_zones > 0 && n_days < (1ll << 31) && n_zones < (1ll << 31), "vs_sst_frame_metrics: sizes must be positive");
    VS_CHECK_ARG(T >= 1 && T <= SM_MAXT, "vs_sst_frame_metrics: 1..%d frames per window (got %d)", SM_MAXT, T);
    VS_CHECK_ARG(rows * T < (1ll << 31), "vs_sst_frame_metrics: rows * T must stay below 2^31");
    VS_CHECK_ARG(H >= MM_WIN && W >= MM_WIN, "vs_sst_frame_metrics: planes of at least %d x %d (got %d x %d)", MM_WIN, MM_WIN, H, W);
    VS_CHECK_ARG(sigma > 0.f, "vs_sst_frame_metrics: sigma must be positive");
    const size_t lds = ((size_t)2 * H * W + (size_t)5 * H * (W - MM_WIN + 1)) * sizeof(float);
    if (lds > 150 * 1024)
        return vs_fail(VS_ERR_UNSUPPORTED, "vs_sst_frame_metrics: planes of %d x %d do not fit the LDS (<= 64 x 64 .. 80 x 80)", H, W);
    MmWindow win;                                    // the window of vs_frame_metrics
    double sum = 0.0, e[MM_WIN];
    for (int j = 0; j < MM_WIN; ++j) {
        const double x = (double)j - (MM_WIN - 1) / 2.0;
        e[j] = exp(-x * x / (2.0 * (double)sigma * (double)sigma));
        sum += e[j];
    }
    for (int j = 0; j < MM_WIN; ++j) win.g[j] = (float)(e[j] / sum);
    const float c1 = k1 * k1, c2 = k2 * k2;          // max_val = 1: the planes are rescaled to the zone's range
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)sst_frame_metrics_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024) != hipSuccess)
            return vs_fail(VS_ERR_LAUNCH, "vs_sst_frame_metrics: cannot raise the dynamic LDS limit");
        attr_set = true;
    }
    hipLaunchKernelGGL(sst_frame_metrics_kernel, dim3((unsigned)(rows * T)), dim3(256), lds, (hipStream_t)stream, pred, target, T, H, W, consts, n_days,
                       (const int*)day0, (const int*)zone, zone_range, n_zones, win, c1, c2, mse, ssim, (int*)bad);
    VS_CHECK_LAUNCH("vs_sst_frame_metrics");
    return VS_OK;
}

// vs_data.hip -- input pipeline on the device: Moving-MNIST sequence generation (reference: data/moving_mnist.py:112-253), the 3D
// Chairs batch gather (reference: data/chairs.py:45-64) and the table-driven window gather of the TaxiBJ timeline (reference:
// data/taxibj.py:74-100), both at the end of this file.
//
// The reference builds every training sequence on the host: per digit five draws from the global NumPy stream (digit index, start
// position, speed), a trajectory of `seq_len` positions with elastic bounces off the frame borders computed in Python floats
// (= IEEE double), and a compositing loop that adds the 28x28 digit into a 64x64 frame per time step, clips at 255 and divides by
// 255.  At MI355X step rates (Moving-MNIST B=128: > 100 k frames/s) a 4-worker host generator is the bottleneck, so here only the
// five integers per digit cross PCIe (drawn by the host from the same NumPy stream, in the reference's order) and one launch
// renders the whole batch:
//   * trajectory: thread d < num_digits of every workgroup replays moving_mnist.py:154-237 for its digit in double arithmetic,
//     operation for operation (deterministic mode: no draws inside the bounce loop), and leaves the rounded positions
//     (Python round() = round-half-even = rint) of frame t in LDS;
//   * compositing: the workgroup of (sample b, frame t) writes the 64x64 frame: sum of the digits' pixels at their positions,
//     min(., 255), / 255 (IEEE division: same bits as NumPy's float32 division), as fp32 or a 16-bit type.
// Digits live in HBM as uint8 [n_digits_total, h, w] (MNIST: 47 MB).
#include "vs_common.h"

namespace {

constexpr int MM_MAXD = 8;          // digits per video (reference default 2)

struct Traj { double sx, sy; int dx, dy; };

// moving_mnist.py:257-299: intersection of the line y = a x + b with a vertical / horizontal border
__device__ __forceinline__ bool inter_x(double a, double b, double x_lim, double lo, double hi, double eps, double& cx, double& cy) {
    const double y = a * x_lim + b;
    cx = x_lim; cy = y;
    return (y >= lo - eps) && (y <= hi + eps);
}
__device__ __forceinline__ bool inter_y(double a, double b, double y_lim, double lo, double hi, double eps, double& cx, double& cy) {
    const double x = (y_lim - b) / a;
    cx = x; cy = y_lim;
    return (x >= lo - eps) && (x <= hi + eps);
}

// moving_mnist.py:177-255 (`_process_collision`, deterministic: the speed is mirrored, never redrawn)
__device__ void process_collision(Traj& s, double x_min, double x_max, double y_min, double y_max) {
    const double eps = 1e-8;
    bool left = s.sx < x_min - eps, upper = s.sy < y_min - eps, right = s.sx > x_max + eps, bottom = s.sy > y_max + eps;
    int guard = 0;
    while ((left || right || upper || bottom) && ++guard < 64) {
        double cx = 0.0, cy = 0.0;
        if (s.dx == 0) {
            cx = s.sx; cy = upper ? y_min : y_max;
        } else if (s.dy == 0) {
            cx = left ? x_min : x_max; cy = s.sy;
        } else {
            const double a = (double)s.dy / (double)s.dx;
            const double b = s.sy - a * s.sx;
            double tx, ty;
            if (left) { left = inter_x(a, b, x_min, y_min, y_max, eps, tx, ty); if (left) { cx = tx; cy = ty; } }
            if (right) { right = inter_x(a, b, x_max, y_min, y_max, eps, tx, ty); if (right) { cx = tx; cy = ty; } }
            if (upper) { upper = inter_y(a, b, y_min, x_min, x_max, eps, tx, ty); if (upper) { cx = tx; cy = ty; } }
            if (bottom) { bottom = inter_y(a, b, y_max, x_min, x_max, eps, tx, ty); if (bottom) { cx = tx; cy = ty; } }
        }
        const double p = s.dx != 0 ? (s.sx - cx) / (double)s.dx : (s.sy - cy) / (double)s.dy;
        if (left) s.dx = abs(s.dx);
        if (right) s.dx = -abs(s.dx);
        if (upper) s.dy = abs(s.dy);
        if (bottom) s.dy = -abs(s.dy);
        s.sx = cx + (double)s.dx * p;
        s.sy = cy + (double)s.dy * p;
        left = s.sx < x_min - eps; upper = s.sy < y_min - eps; right = s.sx > x_max + eps; bottom = s.sy > y_max + eps;
    }
}

// grid (T, B): one workgroup per frame.  init[b][d] = (digit index, sx, sy, dx, dy)
__global__ __launch_bounds__(256) void moving_mnist_kernel(const unsigned char* __restrict__ digits, int dh, int dw, const int* __restrict__ init,
                                                           int nd, int T, int F, void* out, int od) {
    __shared__ int pos[MM_MAXD][3];            // digit index, row offset, column offset of this frame
    const int t = blockIdx.x, b = blockIdx.y;
    if ((int)threadIdx.x < nd) {
        const int* q = init + ((int64_t)b * nd + threadIdx.x) * 5;
        Traj s{(double)q[1], (double)q[2], q[3], q[4]};
        const double x_max = (double)(F - dh), y_max = (double)(F - dw);
        int px = 0, py = 0;
        for (int tt = 0; tt <= t; ++tt) {      // moving_mnist.py:166-175: bounce, record the rounded position, then move
            process_collision(s, 0.0, x_max, 0.0, y_max);
            px = (int)rint(s.sx); py = (int)rint(s.sy);
            s.sy += (double)s.dy;
            s.sx += (double)s.dx;
        }
        pos[threadIdx.x][0] = q[0]; pos[threadIdx.x][1] = px; pos[threadIdx.x][2] = py;
    }
    __syncthreads();
    const int64_t base = ((int64_t)b * T + t) * F * F;
    for (int i = threadIdx.x; i < F * F; i += 256) {
        const int r = i / F, c = i - r * F;
        float v = 0.f;
        for (int d = 0; d < nd; ++d) {
            const int rr = r - pos[d][1], cc = c - pos[d][2];
            if (rr >= 0 && rr < dh && cc >= 0 && cc < dw) v += (float)digits[((int64_t)pos[d][0] * dh + rr) * dw + cc];
        }
        v = v > 255.f ? 255.f : v;
        vs_st(out, od, base + i, v / 255.f);
    }
}

// ---- 3D Chairs: batch gather from the decoded views resident in HBM (data/chairs.py:45-64) ----------------------------------------
// The reference opens and decodes seq_len PNG files per item on the host, stacks them HWC, divides by 255 in float64, rounds to float32
// and permutes to CHW.  Here every view of the split is decoded once and kept as uint8 [n_objects][views][H][W][C]; a batch is one
// launch: grid (seq_len, rows), one workgroup per output frame.  desc[row] = (object, first view); frame t is view
// (first + t) % views (chairs.py:56-57).  (float)byte / 255.f as an IEEE division has, for all 256 bytes, the bits of the reference's
// float64 division rounded to float32.
//
// C == 3 (the dataset): a thread owns PIX consecutive pixels = 3 * PIX consecutive bytes of the HWC frame (PIX = 4 for fp32 output: 12 B,
// PIX = 8 for 16-bit output: 24 B), so a wave reads one contiguous 768 B / 1536 B span, and stores one 16 B vector per channel plane: a
// wave writes 1 KiB contiguous per plane.  Both sides are coalesced without an LDS pass: the transposition is a register shuffle of the
// thread's own bytes.  Other channel counts or H * W not a multiple of PIX take the element-wise form.
template <int PIX, bool LOWP>
__device__ __forceinline__ void chairs_frame_c3(const unsigned char* __restrict__ src, void* out, int64_t obase, int hw, int od) {
    constexpr int NW = 3 * PIX / 4;
    for (int g = threadIdx.x; g < hw / PIX; g += blockDim.x) {
        unsigned int w[NW];
        const unsigned int* p = reinterpret_cast<const unsigned int*>(src) + (int64_t)g * NW;
#pragma unroll
        for (int j = 0; j < NW; ++j) w[j] = p[j];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[PIX];
#pragma unroll
            for (int k = 0; k < PIX; ++k) {
                const int byte = 3 * k + c;
                v[k] = __fdiv_rn((float)((w[byte >> 2] >> (8 * (byte & 3))) & 0xffu), 255.f);
            }
            const int64_t o = obase + (int64_t)c * hw + (int64_t)g * PIX;
            if constexpr (!LOWP) {
                f32x4 q = {v[0], v[1], v[2], v[3]};
                *reinterpret_cast<f32x4*>((float*)out + o) = q;
            } else {
                u16x8 q;
#pragma unroll
                for (int k = 0; k < PIX; ++k) q[k] = vs_f2h(v[k], od);
                *reinterpret_cast<u16x8*>((unsigned short*)out + o) = q;
            }
        }
    }
}

__global__ __launch_bounds__(256) void chairs_gather_kernel(const unsigned char* __restrict__ frames, int64_t n_objects, int views, int hw, int C,
                                                            const int* __restrict__ desc, int T, void* out, int od, int vec, int* bad) {
    const int t = blockIdx.x;
    const int64_t row = blockIdx.y;
    const int obj = desc[row * 2], first = desc[row * 2 + 1];
    const bool ok = obj >= 0 && (int64_t)obj < n_objects && first >= 0 && first < views;        // uniform over the workgroup
    const int64_t fe = (int64_t)hw * C;
    const int64_t obase = (row * T + t) * fe;
    if (!ok) {                                           // the row is written as zeros, nothing is read
        if (bad && threadIdx.x == 0) *bad = 1;
        for (int64_t i = threadIdx.x; i < fe; i += blockDim.x) vs_st(out, od, obase + i, 0.f);
        return;
    }
    const unsigned char* src = frames + ((int64_t)obj * views + ((int64_t)first + t) % views) * fe;
    if (vec) {
        if (od == VS_F32) chairs_frame_c3<4, false>(src, out, obase, hw, od);
        else chairs_frame_c3<8, true>(src, out, obase, hw, od);
        return;
    }
    for (int64_t i = threadIdx.x; i < fe; i += blockDim.x) {       // out element (c, pix) <- byte pix * C + c
        const int64_t c = i / hw, pix = i - c * hw;
        vs_st(out, od, obase + i, __fdiv_rn((float)src[pix * C + c], 255.f));
    }
}

// ---- table-driven window gather from a timeline of frames resident in HBM (data/taxibj.py of the reference: STMatrix.create_dataset) --
// The reference materialises every window on the host; its windows are a SPARSE set (none crosses a missing slot, an incomplete day or a
// file boundary) and each is stored NEWEST FRAME FIRST.  Here the normalised frames live in HBM once as fp32 [n_frames][frame] and a window
// is an entry of a device table: first[w] = index of the frame at position 0; position k is frame first[w] + k * step, step = +1 or -1.
// A batch is one launch driven by the sampler's item indices: out[r, k, :] = frames[first[item[r]] + k * step, :].
// grid (chunks of a row, rows).  A row whose item index is outside [0, n_windows), or whose window would leave [0, n_frames) at either
// end, reads nothing, is written as zeros and raises *bad (the condition is uniform over the workgroup).
// frame % 4 == 0 and aligned bases (`vec`): a thread moves 16 B per load (a 16 B store, or 8 B of 16-bit output), and no vector crosses a
// frame, so a wave reads 1 KiB contiguous inside one frame; other frame sizes go element by element.
__global__ __launch_bounds__(256) void gather_timeline_kernel(const float* __restrict__ frames, int64_t n_frames, int64_t frame,
                                                              const int* __restrict__ first, int64_t n_windows, int step,
                                                              const int* __restrict__ item, int seq_len, void* out, int od, int vec, int* bad) {
    const int64_t row = blockIdx.y;
    const int idx = item[row];
    bool ok = idx >= 0 && (int64_t)idx < n_windows;
    int64_t f0 = 0;
    if (ok) {
        f0 = first[idx];
        const int64_t last = f0 + (int64_t)(seq_len - 1) * step;
        ok = f0 >= 0 && f0 < n_frames && last >= 0 && last < n_frames;
    }
    const int64_t total = (int64_t)seq_len * frame;
    const int64_t obase = row * total;
    if (!ok) {                                           // the row is written as zeros, nothing is read
        if (bad && blockIdx.x == 0 && threadIdx.x == 0) *bad = 1;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) vs_st(out, od, obase + i, 0.f);
        return;
    }
    if (vec) {
        for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < total; i += (int64_t)gridDim.x * 1024) {
            const int64_t k = i / frame, p = i - k * frame;
            const f32x4 v = *reinterpret_cast<const f32x4*>(frames + (f0 + k * step) * frame + p);
            if (od == VS_F32) *reinterpret_cast<f32x4*>((float*)out + obase + i) = v;
            else { const u16x4 w = {vs_f2h(v[0], od), vs_f2h(v[1], od), vs_f2h(v[2], od), vs_f2h(v[3], od)}; *reinterpret_cast<u16x4*>((unsigned short*)out + obase + i) = w; }
        }
        return;
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t k = i / frame, p = i - k * frame;
        vs_st(out, od, obase + i, frames[(f0 + k * step) * frame + p]);
    }
}

}  // namespace

extern "C" int vs_gather_timeline(const float* frames, int64_t n_frames, int64_t frame_elems, const int32_t* first, int64_t n_windows, int step,
                                  const int32_t* item_idx, int64_t rows, int seq_len, void* out, int out_dtype, int32_t* bad, void* stream) {
    VS_CHECK_ARG(frames && first && item_idx && out, "vs_gather_timeline: null pointer");
    VS_CHECK_ARG(n_frames > 0 && frame_elems > 0 && n_windows > 0 && rows > 0, "vs_gather_timeline: sizes must be positive");
    VS_CHECK_ARG(seq_len >= 1, "vs_gather_timeline: seq_len >= 1");
    VS_CHECK_ARG(step == 1 || step == -1, "vs_gather_timeline: step must be +1 or -1 (got %d)", step);
    VS_CHECK_ARG(vs_dtype_ok(out_dtype), "vs_gather_timeline: bad out_dtype");
    VS_CHECK_ARG(rows < 65536, "vs_gather_timeline: at most 65535 rows per launch");
    // the vector form needs whole 4-element groups per frame and aligned vectors: frame starts are multiples of `frame_elems` from the bases
    const int vec = frame_elems % 4 == 0 && (uintptr_t)frames % 16 == 0 && (uintptr_t)out % (out_dtype == VS_F32 ? 16 : 8) == 0;
    const int64_t total = (int64_t)seq_len * frame_elems;
    int64_t gx = vs_cdiv(total, vec ? 1024 : 256);
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(gather_timeline_kernel, dim3((unsigned)gx, (unsigned)rows), dim3(256), 0, (hipStream_t)stream, frames, n_frames, frame_elems,
                       (const int*)first, n_windows, step, (const int*)item_idx, seq_len, out, out_dtype, vec, (int*)bad);
    VS_CHECK_LAUNCH("vs_gather_timeline");
    return VS_OK;
}

extern "C" int vs_chairs_gather(const uint8_t* frames, int64_t n_objects, int views_per_object, int H, int W, int C, const int32_t* desc, int64_t rows,
                                int seq_len, void* out, int out_dtype, int32_t* bad, void* stream) {
    VS_CHECK_ARG(frames && desc && out, "vs_chairs_gather: null pointer");
    VS_CHECK_ARG(n_objects > 0 && views_per_object > 0 && H > 0 && W > 0 && C > 0 && rows > 0, "vs_chairs_gather: sizes must be positive");
    VS_CHECK_ARG(seq_len >= 1, "vs_chairs_gather: seq_len >= 1");
    VS_CHECK_ARG(vs_dtype_ok(out_dtype), "vs_chairs_gather: bad out_dtype");
    VS_CHECK_ARG(rows < 65536, "vs_chairs_gather: at most 65535 rows per launch");
    VS_CHECK_ARG((int64_t)H * W * C < (1ll << 31), "vs_chairs_gather: a frame of %d x %d x %d exceeds 2^31 bytes", H, W, C);
    const int hw = H * W;
    const int64_t fe = (int64_t)hw * C;
    // the vector form needs whole thread spans per frame and aligned vectors: frame starts are multiples of `fe` from the base pointers
    const int pix = out_dtype == VS_F32 ? 4 : 8;
    const int vec = C == 3 && hw % pix == 0 && (uintptr_t)frames % 4 == 0 && fe % 4 == 0 && (uintptr_t)out % 16 == 0;
    hipLaunchKernelGGL(chairs_gather_kernel, dim3((unsigned)seq_len, (unsigned)rows), dim3(256), 0, (hipStream_t)stream, frames, n_objects,
                       views_per_object, hw, C, desc, seq_len, out, out_dtype, vec, (int*)bad);
    VS_CHECK_LAUNCH("vs_chairs_gather");
    return VS_OK;
}

extern "C" int vs_moving_mnist_batch(const uint8_t* digits, int64_t n_digits_total, int digit_h, int digit_w, const int32_t* init, int batch,
                                     int num_digits, int seq_len, int frame_size, void* out, int out_dtype, void* stream) {
    VS_CHECK_ARG(digits && init && out && n_digits_total > 0 && digit_h > 0 && digit_w > 0 && batch > 0 && seq_len > 0, "vs_moving_mnist_batch: bad argument");
    VS_CHECK_ARG(num_digits >= 1 && num_digits <= MM_MAXD, "vs_moving_mnist_batch: 1..%d digits per video", MM_MAXD);
    VS_CHECK_ARG(frame_size >= digit_h && frame_size >= digit_w, "vs_moving_mnist_batch: the digit does not fit the frame");
    VS_CHECK_ARG(vs_dtype_ok(out_dtype), "vs_moving_mnist_batch: bad out_dtype");
    hipLaunchKernelGGL(moving_mnist_kernel, dim3((unsigned)seq_len, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, digits, digit_h, digit_w, init,
                       num_digits, seq_len, frame_size, out, out_dtype);
    VS_CHECK_LAUNCH("vs_moving_mnist_batch");
    return VS_OK;
}

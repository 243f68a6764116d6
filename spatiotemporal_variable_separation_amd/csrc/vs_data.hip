// vs_data.hip -- input pipeline on the device: Moving-MNIST sequence generation (reference: data/moving_mnist.py:112-253) and the
// Moving-MNIST test set in one launch (reference: preprocessing/mnist/make_test_set.py; below the training generator; walked in the launch,
// or -- the stochastic set -- rendered from positions that vs_mmnist_walk.hip walked), the 3D
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

// ---- the Moving-MNIST TEST set (reference: preprocessing/mnist/make_test_set.py:58-91) ---------------------------------------------------
// Thousands of long videos (5 000 x 100 frames), raw bytes instead of normalised floats, the latents (rounded position and speed per frame)
// as a second output, and the file's time-major layout.  One workgroup per (video, chunk of `chunk_len` frames); with enough videos a chunk
// is the whole video, so each trajectory is walked exactly once:
//   1. thread d < nd walks digit d's trajectory with the arithmetic of moving_mnist_kernel (frames before the chunk are replayed, not
//      recorded) and leaves (row, column) per frame in LDS and (row, column, row speed, column speed) in `latents`;
//   2. the workgroup copies its nd digit images into LDS once (a digit index outside [0, n_digits_total) is never read: zeros);
//   3. per frame every thread builds G consecutive pixels (16 bytes: G = 16 as uint8, 4 as fp32) from the LDS digits and stores them as one
//      16-byte vector: at F = 64 as uint8 a frame is exactly one store per thread, a wave writes 1 KiB contiguous.  When the G pixels
//      share a row (F % G == 0) the row is tested once per digit, and most rows miss a digit.
// Frame (t, v) starts at element t * st + v * sv.  VEC needs F * F % G == 0 and 16-byte aligned frame starts (the entry point decides);
// otherwise the same arithmetic goes element by element.  LDS: int2 pos[chunk_len][nd], then nd * dh * dw digit bytes.
__device__ __forceinline__ unsigned mm_pixel(const int2* pos, const unsigned char* dig, int nd, int dh, int dw, int r, int c) {
    unsigned v = 0;
    for (int d = 0; d < nd; ++d) {
        const int rr = r - pos[d].x, cc = c - pos[d].y;
        if ((unsigned)rr < (unsigned)dh && (unsigned)cc < (unsigned)dw) v += dig[(d * dh + rr) * dw + cc];
    }
    return v > 255u ? 255u : v;
}

// Step 3 for one workgroup: frames t0 .. t0 + len - 1 of video v from the positions and digit images in LDS.  Shared by the walking kernel
// and the placing kernel below, which differ only in where the positions come from.
template <bool FP32, bool VEC>
__device__ __forceinline__ void mm_compose(const int2* pos, const unsigned char* dig, int nd, int dh, int dw, int F, int len, int t0, int v,
                                           void* frames, int64_t st, int64_t sv) {
    const int tid = threadIdx.x;
    const int FF = F * F;
    if constexpr (VEC) {
        constexpr int G = FP32 ? 4 : 16;
        const int gpf = FF / G;
        for (int g = tid; g < len * gpf; g += 256) {
            const int f = g / gpf, p0 = (g - f * gpf) * G;
            const int2* pf = pos + f * nd;
            int r = p0 / F, c = p0 - r * F;
            unsigned px[G];
            if (F % G == 0) {                        // the G pixels share a row: one row test per digit, and most rows miss a digit
#pragma unroll
                for (int k = 0; k < G; ++k) px[k] = 0u;
                for (int d = 0; d < nd; ++d) {
                    const int rr = r - pf[d].x, c0 = c - pf[d].y;
                    if ((unsigned)rr >= (unsigned)dh || c0 >= dw || c0 + G <= 0) continue;
                    const unsigned char* row = dig + (d * dh + rr) * dw;
#pragma unroll
                    for (int k = 0; k < G; ++k)
                        if ((unsigned)(c0 + k) < (unsigned)dw) px[k] += row[c0 + k];
                }
#pragma unroll
                for (int k = 0; k < G; ++k) px[k] = px[k] > 255u ? 255u : px[k];
            } else {
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    px[k] = mm_pixel(pf, dig, nd, dh, dw, r, c);
                    if (++c == F) { c = 0; ++r; }
                }
            }
            const int64_t o = (int64_t)(t0 + f) * st + (int64_t)v * sv + p0;
            if constexpr (FP32) {
                const f32x4 w = {(float)px[0], (float)px[1], (float)px[2], (float)px[3]};
                *reinterpret_cast<f32x4*>((float*)frames + o) = w;
            } else {
                u32x4 w;
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = px[4 * j] | (px[4 * j + 1] << 8) | (px[4 * j + 2] << 16) | (px[4 * j + 3] << 24);
                *reinterpret_cast<u32x4*>((unsigned char*)frames + o) = w;
            }
        }
    } else {
        for (int i = tid; i < len * FF; i += 256) {
            const int f = i / FF, p = i - f * FF;
            const int r = p / F, c = p - r * F;
            const unsigned val = mm_pixel(pos + f * nd, dig, nd, dh, dw, r, c);
            const int64_t o = (int64_t)(t0 + f) * st + (int64_t)v * sv + p;
            if constexpr (FP32) ((float*)frames)[o] = (float)val;
            else ((unsigned char*)frames)[o] = (unsigned char)val;
        }
    }
}

template <bool FP32, bool VEC>
__global__ __launch_bounds__(256) void moving_mnist_testset_kernel(const unsigned char* __restrict__ digits, int64_t n_total, int dh, int dw,
                                                                   const int* __restrict__ init, int n_videos, int nd, int T, int F, int chunks,
                                                                   int chunk_len, void* frames, int64_t st, int64_t sv, int* latents) {
    extern __shared__ int2 mm_lds[];
    const int v = blockIdx.x / chunks, t0 = (blockIdx.x - v * chunks) * chunk_len;
    const int len = T - t0 < chunk_len ? T - t0 : chunk_len;
    int2* pos = mm_lds;
    unsigned char* dig = reinterpret_cast<unsigned char*>(mm_lds + (size_t)chunk_len * nd);
    const int tid = threadIdx.x, dsz = dh * dw;
    if (tid < nd) {
        const int* q = init + ((int64_t)v * nd + tid) * 5;
        Traj s{(double)q[1], (double)q[2], q[3], q[4]};
        const double x_max = (double)(F - dh), y_max = (double)(F - dw);
        for (int tt = 0; tt < t0 + len; ++tt) {      // moving_mnist.py:166-175: bounce, record the rounded position and the speed, then move
            process_collision(s, 0.0, x_max, 0.0, y_max);
            if (tt >= t0) {
                const int px = (int)rint(s.sx), py = (int)rint(s.sy);
                pos[(tt - t0) * nd + tid] = make_int2(px, py);
                if (latents) {
                    int* l = latents + (((int64_t)tt * n_videos + v) * nd + tid) * 4;
                    l[0] = px; l[1] = py; l[2] = s.dx; l[3] = s.dy;
                }
            }
            s.sy += (double)s.dy;
            s.sx += (double)s.dx;
        }
    }
    for (int i = tid; i < nd * dsz; i += 256) {
        const int d = i / dsz;
        const int64_t idx = init[((int64_t)v * nd + d) * 5];
        dig[i] = (idx >= 0 && idx < n_total) ? digits[idx * dsz + (i - d * dsz)] : (unsigned char)0;
    }
    __syncthreads();
    mm_compose<FP32, VEC>(pos, dig, nd, dh, dw, F, len, t0, v, frames, st, sv);
}

// The same frames from STORED positions (the stochastic test set: its trajectories consume the random stream as they go, so one workgroup
// walks them all first, vs_mmnist_walk.hip).  Step 1 becomes a copy: the workgroup's slice of positions [T][n_videos][nd][2] goes to LDS.
// A digit whose index is outside [0, n_total), or which is not wholly inside the frame at a frame of the slice, raises *bad and gets a
// position that no pixel of any frame meets, so it is not drawn there; nothing is read outside `digits` or `positions`.
constexpr int MM_AWAY = 1 << 24;    // r - MM_AWAY < 0 for every row of a frame that passed the entry point's size checks

template <bool FP32, bool VEC>
__global__ __launch_bounds__(256) void moving_mnist_testset_place_kernel(const unsigned char* __restrict__ digits, int64_t n_total, int dh, int dw,
                                                                         const int* __restrict__ positions, const int* __restrict__ digit_idx,
                                                                         int n_videos, int nd, int T, int F, int chunks, int chunk_len, void* frames,
                                                                         int64_t st, int64_t sv, int* bad) {
    extern __shared__ int2 mm_lds[];
    const int v = blockIdx.x / chunks, t0 = (blockIdx.x - v * chunks) * chunk_len;
    const int len = T - t0 < chunk_len ? T - t0 : chunk_len;
    int2* pos = mm_lds;
    unsigned char* dig = reinterpret_cast<unsigned char*>(mm_lds + (size_t)chunk_len * nd);
    const int tid = threadIdx.x, dsz = dh * dw;
    for (int i = tid; i < len * nd; i += 256) {
        const int f = i / nd, d = i - f * nd;
        const int* q = positions + (((int64_t)(t0 + f) * n_videos + v) * nd + d) * 2;
        const int px = q[0], py = q[1];
        const int64_t idx = digit_idx[(int64_t)v * nd + d];
        const bool ok = idx >= 0 && idx < n_total && px >= 0 && py >= 0 && px <= F - dh && py <= F - dw;
        if (!ok && bad) *bad = 1;
        pos[i] = ok ? make_int2(px, py) : make_int2(MM_AWAY, MM_AWAY);
    }
    for (int i = tid; i < nd * dsz; i += 256) {
        const int d = i / dsz;
        const int64_t idx = digit_idx[(int64_t)v * nd + d];
        dig[i] = (idx >= 0 && idx < n_total) ? digits[idx * dsz + (i - d * dsz)] : (unsigned char)0;
    }
    __syncthreads();
    mm_compose<FP32, VEC>(pos, dig, nd, dh, dw, F, len, t0, v, frames, st, sv);
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

namespace {

// What vs_moving_mnist_testset and vs_moving_mnist_testset_place check and decide alike: the sizes, the strides, the split of a video over
// workgroups, the LDS of a workgroup and whether frame starts allow 16-byte stores.  VS_OK, or the code vs_fail returned (nothing launched).
struct MmTestsetPlan { int chunks, chunk_len, vec; size_t lds; };

int mm_testset_plan(const char* me, int64_t n_digits_total, int digit_h, int digit_w, int n_videos, int num_digits, int seq_len, int frame_size,
                    const void* frames, int frames_fp32, int64_t st, int64_t sv, MmTestsetPlan& plan) {
    VS_CHECK_ARG(n_digits_total > 0 && digit_h > 0 && digit_w > 0 && n_videos > 0 && seq_len > 0, "%s: sizes must be positive", me);
    VS_CHECK_ARG(num_digits >= 1 && num_digits <= MM_MAXD, "%s: 1..%d digits per video (got %d)", me, MM_MAXD, num_digits);
    VS_CHECK_ARG(frame_size >= digit_h && frame_size >= digit_w, "%s: a %d x %d digit does not fit a frame of %d", me, digit_h, digit_w, frame_size);
    const int64_t FF = (int64_t)frame_size * frame_size;
    // frames must not overlap: the faster-varying index steps over whole frames, the slower one over the whole extent of the faster one
    bool apart = st > 0 && sv > 0;
    if (apart && seq_len > 1 && n_videos > 1) apart = st <= sv ? (st >= FF && sv >= (int64_t)seq_len * st) : (sv >= FF && st >= (int64_t)n_videos * sv);
    else if (apart && seq_len > 1) apart = st >= FF;
    else if (apart && n_videos > 1) apart = sv >= FF;
    VS_CHECK_ARG(apart, "%s: strides (%lld, %lld) make the %d x %d frames of %lld elements overlap", me, (long long)st, (long long)sv, seq_len,
                 n_videos, (long long)FF);
    // few videos: several workgroups per video, each over a chunk of >= 8 frames, until about two workgroups per CU are in flight
    int chunks = 1;
    if (n_videos < 512) {
        const int64_t want = vs_cdiv(512, n_videos), most = vs_cdiv(seq_len, 8);
        chunks = (int)(want < most ? want : most);
    }
    const int chunk_len = (int)vs_cdiv(seq_len, chunks);
    chunks = (int)vs_cdiv(seq_len, chunk_len);
    VS_CHECK_ARG((int64_t)chunk_len * FF < (1ll << 31) && (int64_t)n_videos * chunks < (1ll << 31),
                 "%s: %d frames of %d x %d per workgroup, or %d x %d workgroups, exceed 2^31", me, chunk_len, frame_size, frame_size, n_videos, chunks);
    const size_t table = (size_t)chunk_len * num_digits * sizeof(int2), images = (size_t)num_digits * digit_h * digit_w;
    if (table + images > 64 * 1024)
        return vs_fail(VS_ERR_UNSUPPORTED, "%s: the position table (%d frames x %d digits: %zu B) and the digit images (%zu B) exceed the 65536 B "
                       "of LDS of a workgroup", me, chunk_len, num_digits, table, images);
    const int esize = frames_fp32 ? 4 : 1;
    plan.chunks = chunks;
    plan.chunk_len = chunk_len;
    plan.vec = FF % (16 / esize) == 0 && (uintptr_t)frames % 16 == 0 && (st * esize) % 16 == 0 && (sv * esize) % 16 == 0;
    plan.lds = table + images;
    return VS_OK;
}

}  // namespace

extern "C" int vs_moving_mnist_testset(const uint8_t* digits, int64_t n_digits_total, int digit_h, int digit_w, const int32_t* init, int n_videos,
                                       int num_digits, int seq_len, int frame_size, void* frames, int frames_fp32, int64_t frame_stride_t,
                                       int64_t frame_stride_v, int32_t* latents, void* stream) {
    const char* me = "vs_moving_mnist_testset";
    VS_CHECK_ARG(digits && init && frames, "%s: null pointer", me);
    MmTestsetPlan plan;
    const int rc = mm_testset_plan(me, n_digits_total, digit_h, digit_w, n_videos, num_digits, seq_len, frame_size, frames, frames_fp32,
                                   frame_stride_t, frame_stride_v, plan);
    if (rc != VS_OK) return rc;
    const dim3 grid((unsigned)((int64_t)n_videos * plan.chunks)), block(256);
#define MM_TESTSET_LAUNCH(FP, VEC)                                                                                                                    \
    hipLaunchKernelGGL((moving_mnist_testset_kernel<FP, VEC>), grid, block, plan.lds, (hipStream_t)stream, digits, n_digits_total, digit_h, digit_w, \
                       (const int*)init, n_videos, num_digits, seq_len, frame_size, plan.chunks, plan.chunk_len, frames, frame_stride_t,             \
                       frame_stride_v, (int*)latents)
    if (frames_fp32) { if (plan.vec) MM_TESTSET_LAUNCH(true, true); else MM_TESTSET_LAUNCH(true, false); }
    else { if (plan.vec) MM_TESTSET_LAUNCH(false, true); else MM_TESTSET_LAUNCH(false, false); }
#undef MM_TESTSET_LAUNCH
    VS_CHECK_LAUNCH(me);
    return VS_OK;
}

extern "C" int vs_moving_mnist_testset_place(const uint8_t* digits, int64_t n_digits_total, int digit_h, int digit_w, const int32_t* positions,
                                             const int32_t* digit_idx, int n_videos, int num_digits, int seq_len, int frame_size, void* frames,
                                             int frames_fp32, int64_t frame_stride_t, int64_t frame_stride_v, int32_t* bad, void* stream) {
    const char* me = "vs_moving_mnist_testset_place";
    VS_CHECK_ARG(digits && positions && digit_idx && frames, "%s: null pointer", me);
    MmTestsetPlan plan;
    const int rc = mm_testset_plan(me, n_digits_total, digit_h, digit_w, n_videos, num_digits, seq_len, frame_size, frames, frames_fp32,
                                   frame_stride_t, frame_stride_v, plan);
    if (rc != VS_OK) return rc;
    const dim3 grid((unsigned)((int64_t)n_videos * plan.chunks)), block(256);
#define MM_PLACE_LAUNCH(FP, VEC)                                                                                                                      \
    hipLaunchKernelGGL((moving_mnist_testset_place_kernel<FP, VEC>), grid, block, plan.lds, (hipStream_t)stream, digits, n_digits_total, digit_h,    \
                       digit_w, (const int*)positions, (const int*)digit_idx, n_videos, num_digits, seq_len, frame_size, plan.chunks, plan.chunk_len, \
                       frames, frame_stride_t, frame_stride_v, (int*)bad)
    if (frames_fp32) { if (plan.vec) MM_PLACE_LAUNCH(true, true); else MM_PLACE_LAUNCH(true, false); }
    else { if (plan.vec) MM_PLACE_LAUNCH(false, true); else MM_PLACE_LAUNCH(false, false); }
#undef MM_PLACE_LAUNCH
    VS_CHECK_LAUNCH(me);
    return VS_OK;
}

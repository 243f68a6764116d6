// vs_data.hip -- input pipeline on the device: the Moving-MNIST renderers (reference: data/moving_mnist.py:112-253 for training batches,
// preprocessing/mnist/make_test_set.py for the test set, test_disentanglement.py:66-86 for the content-swap videos), the 3D Chairs batch
// gather (reference: data/chairs.py:45-64) and the table-driven window gather of the TaxiBJ timeline (reference: data/taxibj.py:74-100),
// both at the end of this file.
//
// The reference builds every Moving-MNIST sequence on the host: per digit five draws from the global NumPy stream (digit index, start
// position, speed), a trajectory of `seq_len` positions with elastic bounces off the frame borders computed in Python floats
// (= IEEE double), and a compositing loop that adds the 28x28 digit into a 64x64 frame per time step and clips at 255; training batches
// are divided by 255, the test file keeps the bytes.  At MI355X step rates (Moving-MNIST B=128: > 100 k frames/s) a 4-worker host
// generator is the bottleneck, so here only integers reach the device (the five per digit, or tables of positions) and one launch
// renders all videos.  Four entry points, ONE body.  A workgroup owns (video, chunk of `chunk_len` frames) and
//   1. a LOADER leaves the digits' (row, column) per frame of the chunk in LDS.  WALK (vs_moving_mnist_batch, vs_moving_mnist_testset):
//      thread d < nd walks digit d from `init` with the deterministic sampler of vs_mmnist_bounce_core.h (double arithmetic, operation for
//      operation the reference's; frames before the chunk are replayed, not recorded) and, if asked, writes (row, column, row speed,
//      column speed) to `latents`.  TABLE (vs_moving_mnist_place, vs_moving_mnist_testset_place): a copy from positions
//      [T][n_seq][nd][2], the video's sequence and digits named by a row of an index table; a sequence or digit index out of range, or a
//      digit not wholly inside the frame, raises *bad and gets a position that no pixel of any frame meets, so it is not drawn;
//   2. the workgroup copies its nd digit images into LDS once (a digit index outside [0, n_digits_total) is never read: zeros);
//   3. the COMPOSITOR (mm_compose): per frame every thread builds G consecutive pixels (16 bytes: G = 16 as uint8, 8 as a 16-bit type, 4
//      as fp32) from the LDS digits -- sum, min(., 255), and for the normalised forms / 255 (IEEE division: same bits as NumPy's float32
//      division) -- and stores them as one 16-byte vector: at F = 64 as uint8 a frame is exactly one store per thread, a wave writes
//      1 KiB contiguous.  When the G pixels share a row (F % G == 0) the row is tested once per digit, and most rows miss a digit.
// Frame (t, v) starts at element t * st + v * sv.  VEC needs F * F % G == 0 and 16-byte aligned frame starts (mm_plan decides from the
// entry point's arguments); otherwise the same arithmetic goes element by element.  LDS: int2 pos[chunk_len][nd], then nd * dh * dw
// digit bytes.  Digits live in HBM as uint8 [n_digits_total, h, w] (MNIST: 47 MB).
#include "vs_common.h"
#include "vs_mmnist_bounce_core.h"

namespace {

constexpr int MM_MAXD = 8;          // digits per video (reference default 2)
constexpr int MM_AWAY = 1 << 24;    // r - MM_AWAY < 0 for every row of a frame that passed mm_plan's size checks

// the output forms: raw values 0..255 as uint8 / fp32 (the test file), values / 255 as fp32 / a 16-bit type (training)
enum { MM_U8, MM_F32, MM_NORM32, MM_NORM16 };
__host__ __device__ constexpr int mm_esize(int form) { return form == MM_U8 ? 1 : form == MM_NORM16 ? 2 : 4; }

// what the two kernels share: sizes, the split of a video over workgroups (mm_plan) and the output.  od: VS_BF16 / VS_F16 for MM_NORM16
struct MmJob {
    const unsigned char* digits;
    int64_t n_total;
    int dh, dw, n_videos, nd, T, F, chunks, chunk_len;
    void* frames;
    int od;
    int64_t st, sv;
};

// the workgroup's share: video v, frames t0 .. t0 + len - 1, and its LDS
struct MmSlice {
    int v, t0, len;
    int2* pos;
    unsigned char* dig;
};

__device__ __forceinline__ MmSlice mm_slice(const MmJob& j, int2* lds) {
    MmSlice s;
    s.v = blockIdx.x / j.chunks;
    s.t0 = (blockIdx.x - s.v * j.chunks) * j.chunk_len;
    s.len = j.T - s.t0 < j.chunk_len ? j.T - s.t0 : j.chunk_len;
    s.pos = lds;
    s.dig = reinterpret_cast<unsigned char*>(lds + (size_t)j.chunk_len * j.nd);
    return s;
}

// step 2: idx[d] is the index of the video's digit d
__device__ __forceinline__ void mm_load_digits(const MmJob& j, unsigned char* dig, const int* idx, int idx_step) {
    const int dsz = j.dh * j.dw;
    for (int i = threadIdx.x; i < j.nd * dsz; i += 256) {
        const int d = i / dsz;
        const int64_t n = idx[d * idx_step];
        dig[i] = (n >= 0 && n < j.n_total) ? j.digits[n * dsz + (i - d * dsz)] : (unsigned char)0;
    }
}

__device__ __forceinline__ unsigned mm_pixel(const int2* pos, const unsigned char* dig, int nd, int dh, int dw, int r, int c) {
    unsigned v = 0;
    for (int d = 0; d < nd; ++d) {
        const int rr = r - pos[d].x, cc = c - pos[d].y;
        if ((unsigned)rr < (unsigned)dh && (unsigned)cc < (unsigned)dw) v += dig[(d * dh + rr) * dw + cc];
    }
    return v > 255u ? 255u : v;
}

template <int OUT>
__device__ __forceinline__ float mm_value(unsigned px) { return OUT == MM_NORM32 || OUT == MM_NORM16 ? __fdiv_rn((float)px, 255.f) : (float)px; }

// step 3 for one workgroup, from the positions and digit images in LDS
template <int OUT, bool VEC>
__device__ __forceinline__ void mm_compose(const MmJob& j, const MmSlice& s) {
    const int tid = threadIdx.x, nd = j.nd, dh = j.dh, dw = j.dw, F = j.F;
    const int FF = F * F;
    if constexpr (VEC) {
        constexpr int G = 16 / mm_esize(OUT);
        const int gpf = FF / G;
        for (int g = tid; g < s.len * gpf; g += 256) {
            const int f = g / gpf, p0 = (g - f * gpf) * G;
            const int2* pf = s.pos + f * nd;
            int r = p0 / F, c = p0 - r * F;
            unsigned px[G];
            if (F % G == 0) {                        // the G pixels share a row: one row test per digit, and most rows miss a digit
#pragma unroll
                for (int k = 0; k < G; ++k) px[k] = 0u;
                for (int d = 0; d < nd; ++d) {
                    const int rr = r - pf[d].x, c0 = c - pf[d].y;
                    if ((unsigned)rr >= (unsigned)dh || c0 >= dw || c0 + G <= 0) continue;
                    const unsigned char* row = s.dig + (d * dh + rr) * dw;
#pragma unroll
                    for (int k = 0; k < G; ++k)
                        if ((unsigned)(c0 + k) < (unsigned)dw) px[k] += row[c0 + k];
                }
#pragma unroll
                for (int k = 0; k < G; ++k) px[k] = px[k] > 255u ? 255u : px[k];
            } else {
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    px[k] = mm_pixel(pf, s.dig, nd, dh, dw, r, c);
                    if (++c == F) { c = 0; ++r; }
                }
            }
            const int64_t o = (int64_t)(s.t0 + f) * j.st + (int64_t)s.v * j.sv + p0;
            if constexpr (OUT == MM_U8) {
                u32x4 w;
#pragma unroll
                for (int q = 0; q < 4; ++q) w[q] = px[4 * q] | (px[4 * q + 1] << 8) | (px[4 * q + 2] << 16) | (px[4 * q + 3] << 24);
                *reinterpret_cast<u32x4*>((unsigned char*)j.frames + o) = w;
            } else if constexpr (OUT == MM_NORM16) {
                u16x8 w;
#pragma unroll
                for (int k = 0; k < G; ++k) w[k] = vs_f2h(mm_value<OUT>(px[k]), j.od);
                *reinterpret_cast<u16x8*>((unsigned short*)j.frames + o) = w;
            } else {
                const f32x4 w = {mm_value<OUT>(px[0]), mm_value<OUT>(px[1]), mm_value<OUT>(px[2]), mm_value<OUT>(px[3])};
                *reinterpret_cast<f32x4*>((float*)j.frames + o) = w;
            }
        }
    } else {
        for (int i = tid; i < s.len * FF; i += 256) {
            const int f = i / FF, p = i - f * FF;
            const int r = p / F, c = p - r * F;
            const unsigned val = mm_pixel(s.pos + f * nd, s.dig, nd, dh, dw, r, c);
            const int64_t o = (int64_t)(s.t0 + f) * j.st + (int64_t)s.v * j.sv + p;
            if constexpr (OUT == MM_U8) ((unsigned char*)j.frames)[o] = (unsigned char)val;
            else if constexpr (OUT == MM_NORM16) ((unsigned short*)j.frames)[o] = vs_f2h(mm_value<OUT>(val), j.od);
            else ((float*)j.frames)[o] = mm_value<OUT>(val);
        }
    }
}

// The WALK loader.  init [n_videos][nd][5] = (digit index, start row, start column, row speed, column speed); latents
// [T][n_videos][nd][4] or null.
template <int OUT, bool VEC>
__global__ __launch_bounds__(256) void mm_walk_kernel(MmJob j, const int* __restrict__ init, int* latents) {
    extern __shared__ int2 mm_lds[];
    const MmSlice s = mm_slice(j, mm_lds);
    const int d = threadIdx.x;
    const int* mine = init + (int64_t)s.v * j.nd * 5;
    if (d < j.nd) {
        const int* q = mine + d * 5;
        vsw_walk_deterministic(j.F - j.dh, j.F - j.dw, q[1], q[2], q[3], q[4], s.t0, s.t0 + s.len, [&](int t, const int32_t* row) {
            s.pos[(t - s.t0) * j.nd + d] = make_int2(row[0], row[1]);
            if (latents) {
                int* l = latents + (((int64_t)t * j.n_videos + s.v) * j.nd + d) * 4;
                l[0] = row[0]; l[1] = row[1]; l[2] = row[2]; l[3] = row[3];
            }
        });
    }
    mm_load_digits(j, s.dig, mine, 5);
    __syncthreads();
    mm_compose<OUT, VEC>(j, s);
}

// The TABLE loader.  positions [>= T][n_seq][nd][2]; row v of idx [n_videos][idx_row] names the video's digits, after its sequence if
// idx_seq (vs_moving_mnist_place's desc), else the sequence is v itself.  Nothing is read outside `digits` or `positions`.
template <int OUT, bool VEC>
__global__ __launch_bounds__(256) void mm_table_kernel(MmJob j, const int* __restrict__ positions, int n_seq, const int* __restrict__ idx,
                                                       int idx_row, int idx_seq, int* bad) {
    extern __shared__ int2 mm_lds[];
    const MmSlice s = mm_slice(j, mm_lds);
    const int* mine = idx + (int64_t)s.v * idx_row;
    const int seq = idx_seq ? mine[0] : s.v;
    mine += idx_seq;
    for (int i = threadIdx.x; i < s.len * j.nd; i += 256) {
        const int f = i / j.nd, d = i - f * j.nd;
        const int64_t n = mine[d];
        bool ok = seq >= 0 && seq < n_seq && n >= 0 && n < j.n_total;
        int px = 0, py = 0;
        if (ok) {
            const int* q = positions + (((int64_t)(s.t0 + f) * n_seq + seq) * j.nd + d) * 2;
            px = q[0]; py = q[1];
            ok = px >= 0 && py >= 0 && px <= j.F - j.dh && py <= j.F - j.dw;
        }
        if (!ok && bad) *bad = 1;
        s.pos[i] = ok ? make_int2(px, py) : make_int2(MM_AWAY, MM_AWAY);
    }
    mm_load_digits(j, s.dig, mine, 1);
    __syncthreads();
    mm_compose<OUT, VEC>(j, s);
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

namespace {

// What the four Moving-MNIST entry points check and decide alike: the sizes, the strides, the split of a video over workgroups, the LDS of
// a workgroup and whether frame starts allow 16-byte stores.  Fills j.chunks and j.chunk_len.  VS_OK, or the code vs_fail returned.
struct MmPlan { int vec; size_t lds; unsigned grid; };

// The test set: few videos get several workgroups each, over chunks of >= 8 frames, until about two workgroups per CU are in flight.
// Training batches are few short videos (B = 128 x 15 frames) and one launch is all the GPU has to do: chunks from one frame up until
// about eight workgroups per CU, which at B = 128 is one workgroup per frame (fp32: 16.7 us, against 19.7 us with chunks of 4 and 27.2 us
// with chunks of 8, profiles/mmnist_render_timing.md).
constexpr int MM_TESTSET_CHUNK = 8, MM_TESTSET_GROUPS = 512, MM_TRAIN_CHUNK = 1, MM_TRAIN_GROUPS = 2048;

int mm_plan(const char* me, MmJob& j, int form, int chunk_min, int groups, MmPlan& plan) {
    VS_CHECK_ARG(j.n_total > 0 && j.dh > 0 && j.dw > 0 && j.n_videos > 0 && j.T > 0, "%s: sizes must be positive", me);
    VS_CHECK_ARG(j.nd >= 1 && j.nd <= MM_MAXD, "%s: 1..%d digits per video (got %d)", me, MM_MAXD, j.nd);
    VS_CHECK_ARG(j.F >= j.dh && j.F >= j.dw, "%s: a %d x %d digit does not fit a frame of %d", me, j.dh, j.dw, j.F);
    const int64_t FF = (int64_t)j.F * j.F, st = j.st, sv = j.sv;
    // frames must not overlap: the faster-varying index steps over whole frames, the slower one over the whole extent of the faster one
    bool apart = st > 0 && sv > 0;
    if (apart && j.T > 1 && j.n_videos > 1) apart = st <= sv ? (st >= FF && sv >= (int64_t)j.T * st) : (sv >= FF && st >= (int64_t)j.n_videos * sv);
    else if (apart && j.T > 1) apart = st >= FF;
    else if (apart && j.n_videos > 1) apart = sv >= FF;
    VS_CHECK_ARG(apart, "%s: strides (%lld, %lld) make the %d x %d frames of %lld elements overlap", me, (long long)st, (long long)sv, j.T,
                 j.n_videos, (long long)FF);
    int chunks = 1;
    if (j.n_videos < groups) {
        const int64_t want = vs_cdiv(groups, j.n_videos), most = vs_cdiv(j.T, chunk_min);
        chunks = (int)(want < most ? want : most);
    }
    j.chunk_len = (int)vs_cdiv(j.T, chunks);
    j.chunks = (int)vs_cdiv(j.T, j.chunk_len);
    VS_CHECK_ARG((int64_t)j.chunk_len * FF < (1ll << 31) && (int64_t)j.n_videos * j.chunks < (1ll << 31),
                 "%s: %d frames of %d x %d per workgroup, or %d x %d workgroups, exceed 2^31", me, j.chunk_len, j.F, j.F, j.n_videos, j.chunks);
    const size_t table = (size_t)j.chunk_len * j.nd * sizeof(int2), images = (size_t)j.nd * j.dh * j.dw;
    if (table + images > 64 * 1024)
        return vs_fail(VS_ERR_UNSUPPORTED, "%s: the position table (%d frames x %d digits: %zu B) and the digit images (%zu B) exceed the 65536 B "
                       "of LDS of a workgroup", me, j.chunk_len, j.nd, table, images);
    const int esize = mm_esize(form);
    plan.vec = FF % (16 / esize) == 0 && (uintptr_t)j.frames % 16 == 0 && (st * esize) % 16 == 0 && (sv * esize) % 16 == 0;
    plan.lds = table + images;
    plan.grid = (unsigned)((int64_t)j.n_videos * j.chunks);
    return VS_OK;
}

int mm_norm_form(int out_dtype) { return out_dtype == VS_F32 ? MM_NORM32 : MM_NORM16; }

}  // namespace

// KERNEL<form, plan.vec> on the plan's grid
#define MM_CASE(KERNEL, FORM, VEC, ...) \
    case 2 * FORM + VEC: hipLaunchKernelGGL((KERNEL<FORM, VEC != 0>), dim3(plan.grid), dim3(256), plan.lds, (hipStream_t)stream, __VA_ARGS__); break;
#define MM_LAUNCH(KERNEL, ...)                                                                                                      \
    switch (2 * form + plan.vec) {                                                                                                  \
        MM_CASE(KERNEL, MM_U8, 0, __VA_ARGS__) MM_CASE(KERNEL, MM_U8, 1, __VA_ARGS__) MM_CASE(KERNEL, MM_F32, 0, __VA_ARGS__)        \
        MM_CASE(KERNEL, MM_F32, 1, __VA_ARGS__) MM_CASE(KERNEL, MM_NORM32, 0, __VA_ARGS__) MM_CASE(KERNEL, MM_NORM32, 1, __VA_ARGS__) \
        MM_CASE(KERNEL, MM_NORM16, 0, __VA_ARGS__) MM_CASE(KERNEL, MM_NORM16, 1, __VA_ARGS__)                                        \
    }                                                                                                                               \
    VS_CHECK_LAUNCH(me);                                                                                                            \
    return VS_OK

extern "C" int vs_moving_mnist_batch(const uint8_t* digits, int64_t n_digits_total, int digit_h, int digit_w, const int32_t* init, int batch,
                                     int num_digits, int seq_len, int frame_size, void* out, int out_dtype, void* stream) {
    const char* me = "vs_moving_mnist_batch";
    VS_CHECK_ARG(digits && init && out, "%s: null pointer", me);
    VS_CHECK_ARG(vs_dtype_ok(out_dtype), "%s: bad out_dtype", me);
    const int64_t FF = (int64_t)frame_size * frame_size;
    MmJob job = {digits, n_digits_total, digit_h, digit_w, batch, num_digits, seq_len, frame_size, 0, 0, out, out_dtype, FF, seq_len * FF};
    MmPlan plan;
    const int form = mm_norm_form(out_dtype), rc = mm_plan(me, job, form, MM_TRAIN_CHUNK, MM_TRAIN_GROUPS, plan);
    if (rc != VS_OK) return rc;
    MM_LAUNCH(mm_walk_kernel, job, (const int*)init, (int*)nullptr);
}

extern "C" int vs_moving_mnist_place(const uint8_t* digits, int64_t n_digits_total, int digit_h, int digit_w, const int32_t* positions, int n_seq,
                                     int num_digits, const int32_t* desc, int n_videos, int seq_len, int frame_size, void* out, int out_dtype,
                                     int32_t* bad, void* stream) {
    const char* me = "vs_moving_mnist_place";
    VS_CHECK_ARG(digits && positions && desc && out, "%s: null pointer", me);
    VS_CHECK_ARG(n_seq > 0, "%s: sizes must be positive", me);
    VS_CHECK_ARG(vs_dtype_ok(out_dtype), "%s: bad out_dtype", me);
    const int64_t FF = (int64_t)frame_size * frame_size;
    MmJob job = {digits, n_digits_total, digit_h, digit_w, n_videos, num_digits, seq_len, frame_size, 0, 0, out, out_dtype, FF, seq_len * FF};
    MmPlan plan;
    const int form = mm_norm_form(out_dtype), rc = mm_plan(me, job, form, MM_TRAIN_CHUNK, MM_TRAIN_GROUPS, plan);
    if (rc != VS_OK) return rc;
    MM_LAUNCH(mm_table_kernel, job, (const int*)positions, n_seq, (const int*)desc, 1 + num_digits, 1, (int*)bad);
}

extern "C" int vs_moving_mnist_testset(const uint8_t* digits, int64_t n_digits_total, int digit_h, int digit_w, const int32_t* init, int n_videos,
                                       int num_digits, int seq_len, int frame_size, void* frames, int frames_fp32, int64_t frame_stride_t,
                                       int64_t frame_stride_v, int32_t* latents, void* stream) {
    const char* me = "vs_moving_mnist_testset";
    VS_CHECK_ARG(digits && init && frames, "%s: null pointer", me);
    MmJob job = {digits, n_digits_total, digit_h, digit_w, n_videos, num_digits, seq_len, frame_size, 0, 0, frames, 0, frame_stride_t,
                 frame_stride_v};
    MmPlan plan;
    const int form = frames_fp32 ? MM_F32 : MM_U8, rc = mm_plan(me, job, form, MM_TESTSET_CHUNK, MM_TESTSET_GROUPS, plan);
    if (rc != VS_OK) return rc;
    MM_LAUNCH(mm_walk_kernel, job, (const int*)init, (int*)latents);
}

extern "C" int vs_moving_mnist_testset_place(const uint8_t* digits, int64_t n_digits_total, int digit_h, int digit_w, const int32_t* positions,
                                             const int32_t* digit_idx, int n_videos, int num_digits, int seq_len, int frame_size, void* frames,
                                             int frames_fp32, int64_t frame_stride_t, int64_t frame_stride_v, int32_t* bad, void* stream) {
    const char* me = "vs_moving_mnist_testset_place";
    VS_CHECK_ARG(digits && positions && digit_idx && frames, "%s: null pointer", me);
    MmJob job = {digits, n_digits_total, digit_h, digit_w, n_videos, num_digits, seq_len, frame_size, 0, 0, frames, 0, frame_stride_t,
                 frame_stride_v};
    MmPlan plan;
    const int form = frames_fp32 ? MM_F32 : MM_U8, rc = mm_plan(me, job, form, MM_TESTSET_CHUNK, MM_TESTSET_GROUPS, plan);
    if (rc != VS_OK) return rc;
    MM_LAUNCH(mm_table_kernel, job, (const int*)positions, n_videos, (const int*)digit_idx, num_digits, 0, (int*)bad);
}

// ---- the test-set file's videos, as loaded: uint8 [T, N, ...] -> the fp32 [N, T, ...] that MovingMNIST keeps ----------------------------
namespace {

// dst fp32 [N, T, inner] = src uint8 [T, N, inner]: one workgroup per (t, n) row, four bytes per thread and turn when src allows word loads.
__global__ __launch_bounds__(256) void u8_tn_to_f32_nt_kernel(const uint8_t* __restrict__ src, int64_t T, int64_t N, int64_t inner,
                                                              float* __restrict__ dst) {
    const int64_t row = blockIdx.x, t = row / N, n = row % N;
    const uint8_t* s = src + row * inner;
    float* d = dst + (n * T + t) * inner;
    if ((((uintptr_t)s) & 3) == 0 && (inner & 3) == 0) {
        for (int64_t w = threadIdx.x; w < (inner >> 2); w += 256) {
            const uint32_t v = reinterpret_cast<const uint32_t*>(s)[w];
            f32x4 o;
            o[0] = (float)(v & 255u); o[1] = (float)((v >> 8) & 255u); o[2] = (float)((v >> 16) & 255u); o[3] = (float)(v >> 24);
            *reinterpret_cast<f32x4*>(d + 4 * w) = o;                      // d is 16-byte aligned: dst is, and inner is a multiple of 4
        }
    } else {
        for (int64_t i = threadIdx.x; i < inner; i += 256) d[i] = (float)s[i];
    }
}

}  // namespace

extern "C" int vs_u8_tn_to_f32_nt(const uint8_t* src, int64_t T, int64_t N, int64_t inner, float* dst, void* stream) {
    VS_CHECK_ARG(src && dst, "vs_u8_tn_to_f32_nt: null pointer");
    VS_CHECK_ARG(T >= 0 && N >= 0 && inner >= 0, "vs_u8_tn_to_f32_nt: sizes must not be negative (T %lld, N %lld, inner %lld)", (long long)T, (long long)N,
                 (long long)inner);
    VS_CHECK_ARG(T == 0 || N <= 2147483647ll / T, "vs_u8_tn_to_f32_nt: %lld x %lld rows exceed the grid limit", (long long)T, (long long)N);
    VS_CHECK_ARG(((uintptr_t)dst & 15) == 0, "vs_u8_tn_to_f32_nt: dst %p is not at a 16-byte boundary", (void*)dst);
    if (T * N == 0 || inner == 0) return VS_OK;
    hipLaunchKernelGGL(u8_tn_to_f32_nt_kernel, dim3((unsigned)(T * N)), dim3(256), 0, (hipStream_t)stream, src, T, N, inner, dst);
    VS_CHECK_LAUNCH("vs_u8_tn_to_f32_nt");
    return VS_OK;
}

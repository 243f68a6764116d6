// vs_resample.hip -- crop + two-pass 8-bit resampling with caller-supplied integer coefficient tables: the arithmetic of PIL's
// `ImagingResample` for 8 bits per channel, which the reference's preprocessing/chairs/gen_chairs.py reaches through
// `img.crop(box).resize(size, Image.LANCZOS)`.  The tables come from ops.lanczos_coeffs (22 fractional bits, rounded on the host in C
// doubles); the device does integer arithmetic only, so the result is PIL's to the last bit:
//     horizontal, over the rows of the box:   tmp[y][xx][c] = clamp8(((1 << 21) + sum_x src[y][xmin(xx) + x][c] * kx[xx][x]) >> 22)
//     vertical, over that uint8 intermediate: out[yy][xx][c] = clamp8(((1 << 21) + sum_y tmp[ymin(yy) + y][xx][c] * ky[yy][y]) >> 22)
// 32-bit accumulation, arithmetic shift (a negative sum gives 0).  The rounding of the intermediate to uint8 is part of the result.
//
// Work split: ONE WORKGROUP PER (IMAGE, BAND OF 16 OUTPUT COLUMNS), 256 threads.  A band needs only its own columns of the horizontal
// result, so the bands of an image exchange nothing; one object of 62 views at 64 output columns is 248 workgroups on the 256 CUs,
// where one workgroup per image would leave three CUs in four idle.  The price is that neighbouring bands re-read the taps they share
// (a band of 16 columns at scale 6.25 reads 138 of the 400 box columns: 1.38 x the box over the four bands, served by L2).
// A launch that would have fewer than 256 workgroups that way (one object of 62 views) uses bands of 8 columns instead: twice the
// workgroups, two per CU, so that one computes while the other waits for its rows (8 columns read 88 of 400: 1.76 x the box).
//
// LDS (dynamic, sized and checked by the host entry):
//   * the band's rows of kx and all of ky, and the clamped bounds of both axes;
//   * `inter`: the horizontal result of the band, uint8 [box_h][band columns * C] -- 400 x 48 B = 19.2 KB for the Chairs shape.  It never
//     leaves the CU;
//   * `stage`: a chunk of input rows, only the byte span [lo, hi) the band's taps cover, loaded with coalesced dword loads (a wave reads
//     256 contiguous bytes of a row).  The global byte offset of a row's first tap is rounded DOWN to a dword and the row keeps its
//     phase (offset & 3) in LDS, so neither box_x0 * C nor W * C has to be a multiple of 4.  A dword that would end past the last byte
//     of `src`, and every dword when `src` itself is not 4-byte aligned, is assembled from guarded byte loads instead.  A thread issues
//     all its loads of a chunk (up to 20 dwords) before it uses the first, and the loads of chunk i + 1 are issued before chunk i is
//     computed: they wait in registers and are stored to LDS after the barrier that ends chunk i.  (Stored one by one as they arrived,
//     the loads serialised; profiles/chairs_resample_timing.md has the times.)
// Horizontal pass: a thread owns one (column, channel) of the band and up to 8 rows of the chunk; the tap loop is outermost and goes
// four taps at a time, so 32 multiply-adds cost one 16-byte coefficient read, 32 byte reads whose offsets (tap x C, C a template
// parameter) are immediates of the read instruction, 32 24-bit multiply-adds and 8 pointer increments.
// Vertical pass: a thread owns one (column, channel) and every G-th output row; byte stores of whole band rows (48 contiguous bytes).
//
// Safety: every bound read from a table is clamped into [0, box extent] and its length into [0, min(ksize, box extent - start)] before
// it is used, so NO table contents can make the kernel read outside the box (hence outside `src`) or outside its LDS arrays; a bad table
// gives wrong bytes.  Coefficients are not checked on the device (ops.lanczos_coeffs checks |k| < 2^23 and the 31-bit sum bound on
// the host); the accumulator is unsigned, so a wild table wraps instead of overflowing.
#include "vs_common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_BAND = 16;                  // output columns per workgroup ...
constexpr int RS_FEW_GROUPS = 256;           // ... and half as many when that gives fewer workgroups than this (one per CU)
constexpr int RS_ROWS = 8;                   // rows of a chunk per thread in the horizontal pass
constexpr int RS_FETCH = 20;                 // dwords a thread holds in flight: 256 x 20 x 4 B is one staging area
constexpr int RS_STAGE_MIN = RS_THREADS * RS_FETCH * 4;      // bytes of the staging area (more when one full box row needs more)
constexpr int RS_LDS_MAX = 160 * 1024;

struct ResampleArgs {
    const uint8_t* src; int64_t total;       // bytes of src
    int H, W, C, box_x0, box_y0, box_w, box_h;
    const int32_t *kx, *bx, *ky, *by;
    int ksize_x, ksize_y, out_w, out_h, bands, band_cols, aligned4;
    int stage_bytes;                         // multiple of 4
    uint8_t* out;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ uint8_t clip8(unsigned acc) {
    const int v = (int)acc >> 22;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// one dword of src at byte offset o (a multiple of 4): a dword load where that is aligned and ends inside src, guarded byte loads otherwise
__device__ __forceinline__ uint32_t load_dword(const ResampleArgs& a, int64_t o) {
    if (a.aligned4 && o + 4 <= a.total) return *reinterpret_cast<const uint32_t*>(a.src + o);
    uint32_t w = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (o + b < a.total) w |= (uint32_t)a.src[o + b] << (8 * b);
    return w;
}

// C is a template parameter: the taps of one (column, channel) are C bytes apart, which then fit the LDS reads' immediate offsets
template <int C>
__global__ __launch_bounds__(RS_THREADS) void resample_u8_kernel(const ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int band = blockIdx.x % a.bands;
    const int64_t img = blockIdx.x / a.bands;
    const int kpx = (a.ksize_x + 3) & ~3;                // pitch of a kx row in LDS: whole 16-byte groups
    const int x0 = band * a.band_cols;
    const int bw = a.out_w - x0 < a.band_cols ? a.out_w - x0 : a.band_cols;
    const int ipr = bw * C;                              // (column, channel) items per row of the band: at most 64
    const int G = RS_THREADS / ipr;                      // row groups: at least 4

    // carve (the host entry sized the launch for bands of RS_BAND columns, the widest; every offset is a multiple of 4)
    int* skx = reinterpret_cast<int*>(smem);
    int* sky = skx + RS_BAND * kpx;
    int* sbx = sky + a.out_h * a.ksize_y;
    int* sby = sbx + 2 * RS_BAND;
    uint8_t* stage = reinterpret_cast<uint8_t*>(sby + 2 * a.out_h);
    uint8_t* inter = stage + a.stage_bytes;

    for (int i = tid; i < bw * kpx; i += RS_THREADS) {
        const int col = i / kpx, t = i - col * kpx;
        skx[i] = t < a.ksize_x ? a.kx[(int64_t)(x0 + col) * a.ksize_x + t] : 0;
    }
    for (int i = tid; i < a.out_h * a.ksize_y; i += RS_THREADS) sky[i] = a.ky[i];
    for (int i = tid; i < bw; i += RS_THREADS) {
        const int lo = clampi(a.bx[2 * (x0 + i)], 0, a.box_w);
        const int room = a.box_w - lo < a.ksize_x ? a.box_w - lo : a.ksize_x;
        sbx[2 * i] = lo;
        sbx[2 * i + 1] = clampi(a.bx[2 * (x0 + i) + 1], 0, room);
    }
    for (int i = tid; i < a.out_h; i += RS_THREADS) {
        const int lo = clampi(a.by[2 * i], 0, a.box_h);
        const int room = a.box_h - lo < a.ksize_y ? a.box_h - lo : a.ksize_y;
        sby[2 * i] = lo;
        sby[2 * i + 1] = clampi(a.by[2 * i + 1], 0, room);
    }
    __syncthreads();

    // the box columns [lo, hi) the band's taps cover
    int lo = a.box_w, hi = 0;
    for (int i = 0; i < bw; ++i) {
        const int s = sbx[2 * i], e = s + sbx[2 * i + 1];
        lo = s < lo ? s : lo;
        hi = e > hi ? e : hi;
    }
    if (hi < lo) hi = lo;
    const int span = (hi - lo) * C;                      // bytes of a row that are needed
    const int pitch = (span + 3 + 3) & ~3;               // + the phase, rounded up to whole dwords: at most the host's full-row pitch
    const int nd = pitch >> 2;
    int R = a.stage_bytes / pitch;                       // rows per chunk: at least 1 (stage_bytes >= the full-row pitch)
    if (R > G * RS_ROWS) R = G * RS_ROWS;

    const int64_t row_bytes = (int64_t)a.W * C;
    const int64_t gb0 = ((img * a.H + a.box_y0) * a.W + a.box_x0 + lo) * C;      // byte offset of row 0's first needed byte
    const int ph0 = (int)(gb0 & 3), phr = (int)(row_bytes & 3);

    const int item = tid % ipr, g = tid / ipr;
    const int xc = item / C, c = item - xc * C;
    const int xmin = sbx[2 * xc], xmax = sbx[2 * xc + 1];
    const int* kp = skx + xc * kpx;                      // 16-byte aligned
    const int tap0 = (xmin - lo) * C + c;
    uint32_t* stage32 = reinterpret_cast<uint32_t*>(stage);
    const int step_rr = RS_THREADS / nd, step_d = RS_THREADS - step_rr * nd;
    const int nchunks = (a.box_h + R - 1) / R;

    // Chunk k is rows [k R, k R + Rc).  Dword idx of a chunk is dword (idx % nd) of its row (idx / nd), so a wave reads 256 contiguous
    // bytes of a row, and it lands at stage32[idx] (pitch = 4 nd).  Turn k of the loop issues the loads of chunk k into registers,
    // computes chunk k - 1 from LDS while they fly, and stores them to LDS between the two barriers.
    uint32_t v[RS_FETCH];
    for (int k = 0; k <= nchunks; ++k) {
        const int r0 = k * R;
        const int Rn = k < nchunks ? (a.box_h - r0 < R ? a.box_h - r0 : R) : 0;      // rows of chunk k (0: past the last)
        const int tot = Rn * nd;
        {
            int idx = tid;
            int rr = idx / nd, d = idx - rr * nd;
#pragma unroll
            for (int i = 0; i < RS_FETCH; ++i) {
                if (idx < tot) v[i] = load_dword(a, ((gb0 + (r0 + rr) * row_bytes) & ~(int64_t)3) + 4 * d);
                idx += RS_THREADS; rr += step_rr; d += step_d;
                if (d >= nd) { d -= nd; ++rr; }
            }
        }
        if (k > 0 && g < G) {
            const int p0 = r0 - R;                       // first row of chunk k - 1, which has R rows unless it is the last
            const int Rc = a.box_h - p0 < R ? a.box_h - p0 : R;
            const uint8_t* p[RS_ROWS];
            unsigned acc[RS_ROWS];
#pragma unroll
            for (int j = 0; j < RS_ROWS; ++j) {
                int rr = g + j * G;
                rr = rr < Rc ? rr : 0;                   // a row past the chunk: compute on row 0, store nothing
                p[j] = stage + rr * pitch + ((ph0 + (p0 + rr) * phr) & 3) + tap0;
                acc[j] = 1u << 21;
            }
            int t = 0;
            for (; t + 4 <= xmax; t += 4) {              // 4 taps: one 16-byte coefficient read, byte reads at immediate offsets
                const int4 k4 = *reinterpret_cast<const int4*>(kp + t);
#pragma unroll
                for (int j = 0; j < RS_ROWS; ++j) {
                    const uint8_t* q = p[j] + t * C;
                    acc[j] += (unsigned)__mul24((int)q[0], k4.x) + (unsigned)__mul24((int)q[C], k4.y) + (unsigned)__mul24((int)q[2 * C], k4.z) +
                              (unsigned)__mul24((int)q[3 * C], k4.w);
                }
            }
            for (; t < xmax; ++t) {
                const int kt = kp[t];
#pragma unroll
                for (int j = 0; j < RS_ROWS; ++j) acc[j] += (unsigned)__mul24((int)p[j][t * C], kt);
            }
#pragma unroll
            for (int j = 0; j < RS_ROWS; ++j) {
                const int rr = g + j * G;
                if (rr < Rc) inter[(p0 + rr) * ipr + item] = clip8(acc[j]);
            }
        }
        __syncthreads();                                 // chunk k - 1 is consumed: the staging area is free
#pragma unroll
        for (int i = 0; i < RS_FETCH; ++i) {
            const int idx = i * RS_THREADS + tid;
            if (idx < tot) stage32[idx] = v[i];
        }
        // rows wider than the usual staging area (more than 20 KB each): the rest of the chunk, one dword at a time
        for (int idx = RS_FETCH * RS_THREADS + tid; idx < tot; idx += RS_THREADS) {
            const int rr = idx / nd, d = idx - rr * nd;
            stage32[idx] = load_dword(a, ((gb0 + (r0 + rr) * row_bytes) & ~(int64_t)3) + 4 * d);
        }
        __syncthreads();
    }

    if (g < G) {
        for (int y = g; y < a.out_h; y += G) {
            const int ymin = sby[2 * y], ymax = sby[2 * y + 1];
            const int* kq = sky + y * a.ksize_y;
            const uint8_t* q = inter + ymin * ipr + item;
            unsigned acc = 1u << 21;
            int t = 0;
            for (; t + 4 <= ymax; t += 4) {              // four independent read pairs in flight, not one
                const uint8_t* q4 = q + t * ipr;
                acc += (unsigned)__mul24((int)q4[0], kq[t]) + (unsigned)__mul24((int)q4[ipr], kq[t + 1]) +
                       (unsigned)__mul24((int)q4[2 * ipr], kq[t + 2]) + (unsigned)__mul24((int)q4[3 * ipr], kq[t + 3]);
            }
            for (; t < ymax; ++t) acc += (unsigned)__mul24((int)q[t * ipr], kq[t]);
            a.out[((img * a.out_h + y) * a.out_w + x0) * C + item] = clip8(acc);
        }
    }
}

}  // namespace

extern "C" int vs_resample_u8(const uint8_t* src, int64_t n, int H, int W, int C, int box_x0, int box_y0, int box_w, int box_h, const int32_t* kx,
                              const int32_t* bx, int ksize_x, const int32_t* ky, const int32_t* by, int ksize_y, int out_w, int out_h, uint8_t* out,
                              void* stream) {
    VS_CHECK_ARG(src && kx && bx && ky && by && out, "vs_resample_u8: null pointer");
    VS_CHECK_ARG(n > 0 && H > 0 && W > 0 && out_w > 0 && out_h > 0, "vs_resample_u8: sizes must be positive (n %lld, image %d x %d, output %d x %d)",
                 (long long)n, H, W, out_w, out_h);
    VS_CHECK_ARG(C >= 1 && C <= 4, "vs_resample_u8: 1..4 channels (got %d)", C);
    VS_CHECK_ARG(box_w > 0 && box_h > 0 && box_x0 >= 0 && box_y0 >= 0 && (int64_t)box_x0 + box_w <= W && (int64_t)box_y0 + box_h <= H,
                 "vs_resample_u8: the box (%d, %d) + %d x %d is not inside the %d x %d image", box_x0, box_y0, box_w, box_h, W, H);
    VS_CHECK_ARG(ksize_x >= 1 && ksize_y >= 1, "vs_resample_u8: ksize >= 1 (got %d, %d)", ksize_x, ksize_y);
    // few images: bands of 8 columns, twice the workgroups, so that a CU has two to overlap (62 views: 496 workgroups instead of 248)
    const int band_cols = n * vs_cdiv(out_w, RS_BAND) < RS_FEW_GROUPS && out_w > RS_BAND / 2 ? RS_BAND / 2 : RS_BAND;
    const int64_t bands = vs_cdiv(out_w, band_cols);
    VS_CHECK_ARG(n * bands <= 2147483647ll, "vs_resample_u8: %lld images x %lld bands exceed the grid limit", (long long)n, (long long)bands);
    // LDS: tables + staging (one full box row at least) + the band's horizontal result
    const int64_t full_pitch = ((int64_t)box_w * C + 6) & ~(int64_t)3;
    const int64_t stage = full_pitch > RS_STAGE_MIN ? full_pitch : RS_STAGE_MIN;
    const int64_t tables = 4 * ((int64_t)RS_BAND * ((ksize_x + 3) & ~3) +(int64_t)out_h * ksize_y + 2 * RS_BAND + 2 * (int64_t)out_h);
    const int64_t inter = ((int64_t)box_h * RS_BAND * C + 3) & ~(int64_t)3;
    const int64_t lds = tables + stage + inter;
    VS_CHECK_ARG(lds <= RS_LDS_MAX,
                 "vs_resample_u8: %lld bytes of LDS needed, %d available: intermediate %d rows x %d columns x %d channels = %lld, staging %lld (box "
                 "width %d), tables %lld (ksize %d, %d; output height %d)",
                 (long long)lds, RS_LDS_MAX, box_h, RS_BAND, C, (long long)inter, (long long)stage, box_w, (long long)tables, ksize_x, ksize_y, out_h);
    ResampleArgs a;
    a.src = src; a.total = n * H * W * C;
    a.H = H; a.W = W; a.C = C; a.box_x0 = box_x0; a.box_y0 = box_y0; a.box_w = box_w; a.box_h = box_h;
    a.kx = kx; a.bx = bx; a.ky = ky; a.by = by;
    a.ksize_x = ksize_x; a.ksize_y = ksize_y; a.out_w = out_w; a.out_h = out_h; a.bands = (int)bands; a.band_cols = band_cols;
    a.aligned4 = (uintptr_t)src % 4 == 0;
    a.stage_bytes = (int)stage;
    a.out = out;
    void (*kfn)(const ResampleArgs) = C == 1 ? resample_u8_kernel<1> : C == 2 ? resample_u8_kernel<2> : C == 3 ? resample_u8_kernel<3> : resample_u8_kernel<4>;
    if (lds > 64 * 1024) {                               // above the default limit of dynamic LDS
        if (hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return vs_fail(VS_ERR_LAUNCH, "vs_resample_u8: cannot raise the dynamic LDS limit to %lld bytes", (long long)lds);
    }
    hipLaunchKernelGGL(kfn, dim3((unsigned)(n * bands)), dim3(RS_THREADS), (size_t)lds, (hipStream_t)stream, a);
    VS_CHECK_LAUNCH("vs_resample_u8");
    return VS_OK;
}

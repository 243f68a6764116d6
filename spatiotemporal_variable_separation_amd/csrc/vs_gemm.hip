// vs_gemm.hip -- LDS-tiled MFMA GEMM for gfx950:  C[m,n] = epi( sum_k A(m,k) * B(n,k) ).
//
// One kernel template serves every dense contraction of the var_sep hot path (Linear forward, input
// gradient, weight gradient; see include/varsep_hip.h).  Design points, all MI355X-specific:
//   * 64-wide wavefronts, 4 waves per workgroup arranged 2x2; every wave owns a (BM/2)x(BN/2) block of C as
//     TMxTN accumulators of the 32x32 MFMA shape (16 fp32 registers per lane each).
//   * compute type bf16 -> v_mfma_f32_32x32x16_bf16, fp32 accumulate;
//     compute type f32  -> v_mfma_f32_32x32x2_f32 (bit-exact fp32 FMA chain, the parity path).
//   * operands may be "R" (reduction index contiguous) or "S" (output index contiguous) in memory.  Tiles
//     are staged global -> registers -> LDS with 16-byte vectors along the contiguous axis and kept in LDS
//     in their NATIVE orientation:  R tiles as [row][BK+pad] read back with ds_read_b128;  S tiles as
//     [k][rows+pad] read back with ds_read_b64_tr_b16 (bf16: the hardware transposing read delivers the
//     k-contiguous fragment the MFMA wants) or plain ds_read_b32 (f32: one element per lane).  No operand is
//     ever transposed in HBM, so the weight-gradient GEMM (both operands "S") costs the same as the forward.
//   * pads are chosen so every LDS read is bank-conflict free (MI355X: 64 banks x 4 B, b128 reads served
//     in 16-lane groups, tr_b16/b64 reads in 32-lane halves).
//   * register prefetch of tile t+1 is issued before the MFMAs of tile t (global latency hides under the
//     matrix pipe); one LDS buffer, two barriers per K tile; 2-4 workgroups per CU overlap each other.
//   * few-tile/long-K problems (encoder first layer: M=128..256, K=20480) are split along K over
//     gridDim.z into fp32 slabs and combined by a second kernel that also applies the epilogue, so the
//     result is bitwise reproducible (no float atomics).
#include <type_traits>
#include "vs_gemm_plan.h"
#include "vs_loss.h"

namespace {

// one dense contraction as the launchers see it (problem i of a batch: A + i * epi.batch_a, B + i * epi.batch_b)
struct GemmCall {
    const void* A; int64_t lda; int la;
    const void* B; int64_t ldb; int lb;
    int64_t M, N, K;
    int batch;
    hipStream_t stream;
};

// runtime compute type / operand layouts -> template arguments: f(IC<CT>) and f(IC<CT>, IC<LA>, IC<LB>)
template <int V> using IC = std::integral_constant<int, V>;
template <class F>
int with_compute(int compute, F&& f) {
    return compute == VS_BF16 ? f(IC<VS_BF16>{}) : compute == VS_F16 ? f(IC<VS_F16>{}) : f(IC<VS_F32>{});
}
template <class F>
int with_types(int compute, int la, int lb, F&& f) {
    return with_compute(compute, [&](auto ct) {
        if (la == LR && lb == LR) return f(ct, IC<LR>{}, IC<LR>{});
        if (la == LR && lb == LS) return f(ct, IC<LR>{}, IC<LS>{});
        if (la == LS && lb == LR) return f(ct, IC<LS>{}, IC<LR>{});
        return f(ct, IC<LS>{}, IC<LS>{});
    });
}

template <int CT, int LA, int LB, int BM, int BN>
int launch(const GemmCall& c, const GemmPlan& plan, const Epi& epi, float* slabs) {
    typedef typename CTraits<CT>::T T;
    constexpr int BK = bk_of<CT>();
    constexpr int U = CTraits<CT>::U;
    // 16-byte vector loads need every problem of a batch to start 16-byte aligned too
    Dense<CT, LA> a{(const T*)c.A, c.lda, c.M, c.K, ((uintptr_t)c.A % 16 == 0) && (c.lda % U == 0) && (epi.batch_a % U == 0)};
    Dense<CT, LB> b{(const T*)c.B, c.ldb, c.N, c.K, ((uintptr_t)c.B % 16 == 0) && (c.ldb % U == 0) && (epi.batch_b % U == 0)};
    constexpr size_t smem = (TileGeom<CT, LA, BM, BK>::ELEMS + TileGeom<CT, LB, BN, BK>::ELEMS) * sizeof(T);
    dim3 grid((unsigned)vs_cdiv(c.N, BN), (unsigned)vs_cdiv(c.M, BM), (unsigned)(plan.splits * c.batch));
    // XCD runs (Epi::xcd_runs) from 64 workgroups upwards: PMC on the WaveEq decoder layers (3328 x 1200 x 1200, 988 tiles of 64 x 64) showed
    // 77 MB fetched per launch for 11 MB of operands -- each of the eight L2s pulled the whole of A and B.
    Epi e = epi;
    e.xcd_runs = (int64_t)grid.x * grid.y * grid.z >= 64;
    hipLaunchKernelGGL((gemm_kernel<CT, Dense<CT, LA>, Dense<CT, LB>, BM, BN, BK>), grid, dim3(256), smem, c.stream, a, b, c.M, c.N,
                       c.K, (int)plan.k_tiles_per_split, e, slabs);
    VS_CHECK_LAUNCH("vs_gemm");
    return VS_OK;
}

// the register-staged tile in the shape the plan names (64x128: 16-bit only)
template <int CT, int LA, int LB>
int launch_reg(const GemmCall& c, const GemmPlan& plan, const Epi& epi, float* slabs) {
    if (plan.bm == 128 && plan.bn == 128) return launch<CT, LA, LB, 128, 128>(c, plan, epi, slabs);
    if (plan.bm == 128 && plan.bn == 64) return launch<CT, LA, LB, 128, 64>(c, plan, epi, slabs);
    if constexpr (CT != VS_F32)
        if (plan.bm == 64 && plan.bn == 128) return launch<CT, LA, LB, 64, 128>(c, plan, epi, slabs);
    return launch<CT, LA, LB, 64, 64>(c, plan, epi, slabs);
}

template <int CT, int LA, int LB>
int launch_glds(const GemmCall& c, const GemmPlan& plan, const Epi& epi, float* slabs) {
    if constexpr (CT == VS_F32) {
        return vs_fail(VS_ERR_UNSUPPORTED, "vs_gemm: the LDS-DMA 128x128 tile is a 16-bit kernel");
    } else {
        dim3 grid((unsigned)vs_cdiv(c.N, 128), (unsigned)vs_cdiv(c.M, 128), (unsigned)(plan.splits * c.batch));
        static const int forced = getenv("VS_GEMM_GLDS_STAGES") ? atoi(getenv("VS_GEMM_GLDS_STAGES")) : 0;
        const int stages = forced ? forced : ((int64_t)grid.x * grid.y * grid.z >= 1024 ? 2 : 1);
        if (stages == 2)
            hipLaunchKernelGGL((gemm_glds_kernel<LA, LB, false, 2, CT>), grid, dim3(256), 65536, c.stream, (const __bf16*)c.A, c.lda, (const __bf16*)c.B,
                               c.ldb, c.M, c.N, c.K, (int)plan.k_tiles_per_split, epi, slabs);
        else
            hipLaunchKernelGGL((gemm_glds_kernel<LA, LB, false, 1, CT>), grid, dim3(256), 32768, c.stream, (const __bf16*)c.A, c.lda, (const __bf16*)c.B,
                               c.ldb, c.M, c.N, c.K, (int)plan.k_tiles_per_split, epi, slabs);
        VS_CHECK_LAUNCH("vs_gemm (LDS-DMA tile)");
        return VS_OK;
    }
}

template <int CT, int LA, int LB, bool LOSS = false>
int launch_big(const GemmCall& c, const GemmPlan& bp, const Epi& epi, float* slabs) {
    if constexpr (CT == VS_F32) {
        return vs_fail(VS_ERR_UNSUPPORTED, "vs_gemm: the 256x256 tile is a 16-bit kernel");
    } else {
        auto kfn = gemm_big_kernel<CT, LA, LB, false, LOSS>;
        static bool attr_set = false;                  // 128 KiB of dynamic LDS: above the 64 KiB default limit
        if (!attr_set) {
            if (hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_BIG_STAGES * BIG_TILE_BYTES) != hipSuccess)
                return vs_fail(VS_ERR_LAUNCH, "vs_gemm: cannot raise the dynamic LDS limit to 160 KiB");
            attr_set = true;
        }
        dim3 grid((unsigned)(bp.tiles_m * bp.tiles_n), 1, (unsigned)(bp.splits * c.batch));
        hipLaunchKernelGGL(kfn, grid, dim3(512), GEMM_BIG_STAGES * BIG_TILE_BYTES, c.stream, (const unsigned short*)c.A, c.lda, (const unsigned short*)c.B,
                           c.ldb, c.M, c.N, c.K, (int)bp.k_tiles_per_split, bp.tiles_n, epi, slabs);
        VS_CHECK_LAUNCH("vs_gemm (256x256 tile)");
        return VS_OK;
    }
}

// the 256 x 256 / 256 x 128 tile with two staggered wave groups (vs_gemm_p8.h)
template <int CT, int LA, int LB, int NI, int LOSS = 0, int MI = 4>
int launch_p8(const GemmCall& c, const GemmPlan& pp, const Epi& epi, float* slabs) {
    if constexpr (CT == VS_F32) {
        return vs_fail(VS_ERR_UNSUPPORTED, "vs_gemm: the staggered 256-row tile is a 16-bit kernel");
    } else {
        auto kfn = gemm_p8_kernel<CT, LA, LB, NI, false, LOSS, MI>;
        constexpr int lds = 2 * (2 * 32 * MI * P8_BK * 2 + 2 * 64 * NI * P8_BK * 2);
        static bool attr_set = false;                  // 96 / 128 KiB of dynamic LDS: above the 64 KiB default limit
        if (!attr_set) {
            if (hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
                return vs_fail(VS_ERR_LAUNCH, "vs_gemm: cannot raise the dynamic LDS limit to %d bytes", lds);
            attr_set = true;
        }
        dim3 grid((unsigned)(pp.tiles_m * pp.tiles_n), 1, (unsigned)(pp.splits * c.batch));
        hipLaunchKernelGGL(kfn, grid, dim3(512), lds, c.stream, (const unsigned short*)c.A, c.lda, (const unsigned short*)c.B, c.ldb, c.M, c.N, c.K,
                           (int)pp.k_tiles_per_split, pp.tiles_n, epi, slabs);
        VS_CHECK_LAUNCH("vs_gemm (staggered 256-row tile)");
        return VS_OK;
    }
}

template <int CT, int LA, int LB>
int launch_mid(const GemmCall& c, const GemmPlan& mp, const Epi& epi, float* slabs) {
    const int rc = mid_launch<CT, LA, LB>(c.A, c.lda, c.B, c.ldb, c.M, c.N, c.K, mp.splits, mp.k_tiles_per_split, mp.stages, c.batch, epi, slabs, c.stream);
    if (rc != VS_OK) return rc;
    VS_CHECK_LAUNCH("vs_gemm (128x128 ring tile)");
    return VS_OK;
}

// the kernel the plan names, for the call's compute type and layouts
int launch_plan(int compute, const GemmCall& c, const GemmPlan& p, const Epi& epi, float* slabs) {
    return with_types(compute, c.la, c.lb, [&](auto ct, auto la, auto lb) -> int {
        constexpr int CT = decltype(ct)::value, LA = decltype(la)::value, LB = decltype(lb)::value;
        switch (p.kind) {
            case GEMM_P8:
                if (p.ni == 1 && p.mi == 2) return launch_p8<CT, LA, LB, 1, 0, 2>(c, p, epi, slabs);
                if (p.ni == 1) return launch_p8<CT, LA, LB, 1>(c, p, epi, slabs);
                return launch_p8<CT, LA, LB, 2>(c, p, epi, slabs);
            case GEMM_BIG: return launch_big<CT, LA, LB>(c, p, epi, slabs);
            case GEMM_MID: return launch_mid<CT, LA, LB>(c, p, epi, slabs);
            case GEMM_GLDS: return launch_glds<CT, LA, LB>(c, p, epi, slabs);
            default: return launch_reg<CT, LA, LB>(c, p, epi, slabs);
        }
    });
}

// ---- split-K arrival counters -------------------------------------------------------------------------------------------------
// One word per output tile of a split launch, zero between launches (the last workgroup to arrive clears it).  The words come from a static
// pool in device memory (no allocation behind the ABI), dealt out round robin: two launches share a word only if more than SK_POOL words
// were taken between them AND they are in flight at the same time; a recorded graph keeps the ranges it was captured with.
constexpr unsigned SK_POOL = 1u << 20;
}  // namespace
__device__ unsigned vs_sk_pool[1u << 20];         // (external linkage: hipGetSymbolAddress does not find a symbol of an unnamed namespace)
namespace {

// `tile_slab_bytes`: what the last workgroup of a tile has to read back (splits x tile x 4 B).  It reads at ~16-64 KB per us (one workgroup,
// dependent on the loads it keeps in flight), the reduce launch at TB/s: the fix-up pays for small tiles x few splits only (measured in the
// WaveEq step: 256 x 1200 x 20480 in 22 splits of 128 x 128 tiles, 1.4 MB per tile: 41 -> 115 us; 64 x 64 tiles x 4 splits: even or ahead).
// With the threshold the WaveEq step is still 15-25 us SLOWER (1.284 / 1.286 / 1.299 vs 1.268 / 1.268 / 1.275 ms, three interleaved pairs: the
// 64 x 64 kernel's slabs leave as 4-byte sc1 stores, one fabric write each), so the fix-up is OPT-IN: VS_GEMM_SPLITK_FUSED: 0 = never (default),
// 1 = up to SK_FUSED_MAX_BYTES per tile, 2 = always.
constexpr int64_t SK_FUSED_MAX_BYTES = 96 << 10;
unsigned* sk_take(int64_t words, int64_t tile_slab_bytes) {
    static unsigned* base = nullptr;
    static unsigned next = 0;
    const char* env = getenv("VS_GEMM_SPLITK_FUSED");              // read per call: tests switch it
    const int fused = env ? atoi(env) : 0;
    if (!fused || words <= 0 || words > SK_POOL / 4 || (fused == 1 && tile_slab_bytes > SK_FUSED_MAX_BYTES)) return nullptr;
    if (!base && hipGetSymbolAddress((void**)&base, HIP_SYMBOL(vs_sk_pool)) != hipSuccess) { base = nullptr; return nullptr; }
    if (next + words > SK_POOL) next = 0;
    unsigned* p = base + next;
    next += (unsigned)words;
    return p;
}

// One planned contraction: slab check, arrival counters, the launch, the reduce launch.  `who` prefixes the error text.
int run_gemm(const char* who, int compute, const GemmCall& c, const GemmPlan& plan, Epi epi, void* workspace, size_t workspace_bytes) {
    float* slabs = nullptr;
    if (plan.splits > 1) {
        const size_t need = gemm_slab_bytes(plan, c.M, c.N, c.batch);
        if (!workspace || workspace_bytes < need)
            return vs_fail(VS_ERR_WORKSPACE, "%s: split-K needs %zu workspace bytes, got %zu", who, need, workspace_bytes);
        slabs = (float*)workspace;
        if (gemm_splitk_in_launch(plan)) {
            epi.sk_counters = sk_take(gemm_splitk_counters(plan, c.M, c.N, c.batch), gemm_splitk_tile_bytes(plan));
            epi.sk_splits = plan.splits;
            epi.sk_bytes = (int64_t)need;
        }
    }
    const int rc = launch_plan(compute, c, plan, epi, slabs);
    if (rc != VS_OK) return rc;
    if (slabs && !epi.sk_counters) return launch_splitk_reduce(slabs, plan.splits, c.M, c.N, epi, c.batch, c.stream);
    return VS_OK;
}

}  // namespace

extern "C" size_t vs_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K) { return gemm_workspace_bytes(M, N, K, 1); }
extern "C" size_t vs_gemm_batched_workspace_bytes(int batch, int64_t M, int64_t N, int64_t K) { return gemm_workspace_bytes(M, N, K, batch); }

// Host-only view of the decision vs_gemm / vs_gemm_batched take for these arguments: plan_gemm, printed.  No GPU call; the operand
// addresses are looked at for alignment only.
extern "C" int vs_gemm_plan(int compute, int batch, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, int64_t stride_a, int layout_a,
                            const void* B, int64_t ldb, int64_t stride_b, int layout_b, int64_t* out) {
    VS_CHECK_ARG(vs_dtype_ok(compute), "vs_gemm_plan: compute type %d", compute);
    VS_CHECK_ARG(batch >= 1 && batch <= 1024 && M > 0 && N > 0 && K > 0, "vs_gemm_plan: bad sizes");
    VS_CHECK_ARG((layout_a == LR || layout_a == LS) && (layout_b == LR || layout_b == LS), "vs_gemm_plan: bad layout");
    VS_CHECK_ARG(out, "vs_gemm_plan: null pointer");
    const GemmPlan p = plan_gemm(compute, M, N, K, batch, A, lda, layout_a, stride_a, B, ldb, layout_b, stride_b);
    const int64_t row[12] = {p.kind, p.bm, p.bn, p.splits, p.k_tiles_per_split, p.tiles_m, p.tiles_n, p.stages, p.ni, p.mi,
                             gemm_splitk_in_launch(p) && gemm_splitk_counters(p, M, N, batch) > 0, (int64_t)gemm_slab_bytes(p, M, N, batch)};
    memcpy(out, row, sizeof(row));
    return VS_OK;
}

// `batch` independent problems of one shape in one launch (the weight gradients of the integrator's blocks: the same three
// small GEMMs per block, each too small to fill the chip): problem i uses A + i*stride_a, B + i*stride_b, C + i*stride_c.
extern "C" int vs_gemm_batched(int compute, int batch, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, int64_t stride_a,
                               int layout_a, const void* B, int64_t ldb, int64_t stride_b, int layout_b, void* C, int64_t ldc,
                               int64_t stride_c, int c_dtype, float alpha, int accumulate, void* workspace, size_t workspace_bytes,
                               void* stream_) {
    VS_CHECK_ARG(vs_dtype_ok(compute), "vs_gemm_batched: compute type %d", compute);
    VS_CHECK_ARG(batch >= 1 && batch <= 1024 && M > 0 && N > 0 && K > 0, "vs_gemm_batched: bad sizes");
    VS_CHECK_ARG(A && B && C, "vs_gemm_batched: null operand");
    VS_CHECK_ARG((layout_a == LR || layout_a == LS) && (layout_b == LR || layout_b == LS), "vs_gemm_batched: bad layout");
    VS_CHECK_ARG(vs_dtype_ok(c_dtype), "vs_gemm_batched: bad c_dtype");
    VS_CHECK_ARG(lda >= (layout_a == LR ? K : M) && ldb >= (layout_b == LR ? K : N) && ldc >= N, "vs_gemm_batched: leading dimension too small");
    const GemmPlan plan = plan_gemm(compute, M, N, K, batch, A, lda, layout_a, stride_a, B, ldb, layout_b, stride_b);
    Epi epi = plain_epi(C, ldc, c_dtype, alpha);
    epi.accumulate = accumulate;
    epi.splits_per_batch = plan.splits;            // > 0 marks the batched form for the kernels, even for a batch of 1
    epi.batch_a = stride_a; epi.batch_b = stride_b; epi.batch_c = stride_c;
    const GemmCall call{A, lda, layout_a, B, ldb, layout_b, M, N, K, batch, (hipStream_t)stream_};
    return run_gemm("vs_gemm_batched", compute, call, plan, epi, workspace, workspace_bytes);
}

// Weight gradient + optimizer in one launch: G = A * B^T (as vs_gemm) is the gradient of the fp32 parameter `param` [M, N]; the
// epilogue applies the Adam update (vs_adam_math.h: bitwise what vs_adam_multi computes from a stored G) to param / exp_avg /
// exp_avg_sq and rewrites the 16-bit operand copy.  The gradient never reaches HBM: per parameter 12 B read + 14 B written instead
// of 4 B (gradient store) + 30 B (optimizer pass).  16-bit operands that fit the LDS-DMA loader only (VS_ERR_UNSUPPORTED otherwise:
// the caller falls back to vs_gemm + vs_adam_multi); no split-K, whatever K.
extern "C" int vs_gemm_adam(int compute, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, int layout_a, const void* B, int64_t ldb,
                            int layout_b, float alpha, float* param, float* exp_avg, float* exp_avg_sq, void* shadow, int shadow_dtype,
                            const int32_t* step, int32_t skipped, double lr, double beta1, double beta2, double eps, void* stream_) {
    VS_CHECK_ARG(compute == VS_BF16 || compute == VS_F16, "vs_gemm_adam: 16-bit compute types only (%d)", compute);
    VS_CHECK_ARG(M > 0 && N > 0 && K > 0, "vs_gemm_adam: M, N, K must be positive");
    VS_CHECK_ARG(A && B && param && exp_avg && exp_avg_sq && step, "vs_gemm_adam: null pointer");
    VS_CHECK_ARG((layout_a == LR || layout_a == LS) && (layout_b == LR || layout_b == LS), "vs_gemm_adam: bad layout");
    VS_CHECK_ARG(lda >= (layout_a == LR ? K : M) && ldb >= (layout_b == LR ? K : N), "vs_gemm_adam: leading dimension too small");
    VS_CHECK_ARG(!shadow || shadow_dtype == VS_BF16 || shadow_dtype == VS_F16, "vs_gemm_adam: bad shadow dtype");
    if (!dma_operands_ok(GEMM_MID, A, lda, layout_a, 0, B, ldb, layout_b, 0, M, N, K))
        return vs_fail(VS_ERR_UNSUPPORTED, "vs_gemm_adam: operands do not fit the LDS-DMA loader (16-byte alignment, multiples of 8)");
    Epi epi = plain_epi(param, N, VS_F32, alpha);
    epi.adam_m = exp_avg; epi.adam_v = exp_avg_sq; epi.adam_shadow = (unsigned short*)shadow; epi.adam_shadow_dtype = shadow_dtype;
    epi.adam_step = step; epi.adam_skipped = skipped; epi.adam_guard = vs_g_exchange_guard;
    epi.adam_lr = lr; epi.adam_beta1 = beta1; epi.adam_beta2 = beta2; epi.adam_eps = (float)eps;
    const GemmPlan mp = ring_plan_one_split(M, N, K);
    if ((int64_t)mp.tiles_m * mp.tiles_n > 0x7fffffffll) return vs_fail(VS_ERR_UNSUPPORTED, "vs_gemm_adam: too many tiles");
    const GemmCall call{A, lda, layout_a, B, ldb, layout_b, M, N, K, 1, (hipStream_t)stream_};
    return launch_plan(compute, call, mp, epi, nullptr);
}

// vs_gemm_adam as a launch that is deliberately NOT chip-filling (include/varsep_hip.h): the same tiles, the same arithmetic, bit for bit.
extern "C" int vs_gemm_adam_paced(int compute, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, int layout_a, const void* B, int64_t ldb,
                                  int layout_b, float alpha, float* param, float* exp_avg, float* exp_avg_sq, void* shadow, int64_t ldp,
                                  int shadow_dtype, const int32_t* step, int32_t skipped, double lr, double beta1, double beta2, double eps,
                                  int max_workgroups, int pieces_in_flight, int cache_policy, void* stream_) {
    VS_CHECK_ARG(compute == VS_BF16 || compute == VS_F16, "vs_gemm_adam_paced: 16-bit compute types only (%d)", compute);
    VS_CHECK_ARG(M > 0 && N > 0 && K > 0, "vs_gemm_adam_paced: M, N, K must be positive");
    VS_CHECK_ARG(A && B && param && exp_avg && exp_avg_sq && step, "vs_gemm_adam_paced: null pointer");
    VS_CHECK_ARG((layout_a == LR || layout_a == LS) && (layout_b == LR || layout_b == LS), "vs_gemm_adam_paced: bad layout");
    VS_CHECK_ARG(lda >= (layout_a == LR ? K : M) && ldb >= (layout_b == LR ? K : N) && ldp >= N, "vs_gemm_adam_paced: leading dimension too small");
    VS_CHECK_ARG(!shadow || shadow_dtype == VS_BF16 || shadow_dtype == VS_F16, "vs_gemm_adam_paced: bad shadow dtype");
    VS_CHECK_ARG(max_workgroups >= 1, "vs_gemm_adam_paced: max_workgroups must be positive (%d)", max_workgroups);
    VS_CHECK_ARG(pieces_in_flight == 1 || pieces_in_flight == 2 || pieces_in_flight == 4, "vs_gemm_adam_paced: pieces_in_flight is 1, 2 or 4 (%d)", pieces_in_flight);
    VS_CHECK_ARG(cache_policy == 0 || cache_policy == 1, "vs_gemm_adam_paced: cache_policy is 0 (plain) or 1 (non-temporal) (%d)", cache_policy);
    if (!dma_operands_ok(GEMM_MID, A, lda, layout_a, 0, B, ldb, layout_b, 0, M, N, K))
        return vs_fail(VS_ERR_UNSUPPORTED, "vs_gemm_adam_paced: operands do not fit the LDS-DMA loader (16-byte alignment, multiples of 8)");
    if ((((uintptr_t)param | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0 || ((uintptr_t)shadow & 7) != 0 || (ldp & 3) != 0)
        return vs_fail(VS_ERR_UNSUPPORTED, "vs_gemm_adam_paced: parameter and moments 16-byte aligned, operand copy 8-byte aligned, ldp a multiple of 4");
    if (vs_cdiv(M, 128) * vs_cdiv(N, 128) > 0x7fffffffll) return vs_fail(VS_ERR_UNSUPPORTED, "vs_gemm_adam_paced: too many tiles");
    Epi epi = plain_epi(param, ldp, VS_F32, alpha);
    epi.adam_m = exp_avg; epi.adam_v = exp_avg_sq; epi.adam_shadow = (unsigned short*)shadow; epi.adam_shadow_dtype = shadow_dtype;
    epi.adam_step = step; epi.adam_skipped = skipped; epi.adam_guard = vs_g_exchange_guard;
    epi.adam_lr = lr; epi.adam_beta1 = beta1; epi.adam_beta2 = beta2; epi.adam_eps = (float)eps;
    const int rc = with_types(compute, layout_a, layout_b, [&](auto ct, auto la, auto lb) -> int {
        return mid_launch_paced<decltype(ct)::value, decltype(la)::value, decltype(lb)::value>(A, lda, B, ldb, M, N, K, epi, max_workgroups, pieces_in_flight,
                                                                                                cache_policy, (hipStream_t)stream_);
    });
    if (rc != VS_OK) return rc;
    VS_CHECK_LAUNCH("vs_gemm_adam_paced");
    return VS_OK;
}

// The decoder's last Linear layer with the frame losses in its epilogue (recorded MLP-family step): frames = act(A W^T + bias) is row
// r = (b, g) of the decoded stack [B, G, N = D] (reference: networks/mlp_encdec.py:43-50 + train.py:85-86, 139); instead of storing the
// 54 MB of fp32 frames and reading them back with the targets (vs_train_losses_fwd_grad), the 256 x 256 tile kernel compares its result
// with full[b, target(g)] while it is in registers: squared errors into one partial-sum pair per workgroup, k (y - target) act'(y) into
// `dz`.  A one-workgroup launch then adds the partials, computes the two code terms and their gradients and assembles `out` (layout of
// vs_train_losses_fwd_grad: [4] total, [5] ae, [6] zero-order, [7] pred, [8] t_reg).  VS_ERR_UNSUPPORTED when the problem does not run on
// the 256 x 256 tile (the caller stores the frames and calls vs_train_losses_fwd_grad instead).
extern "C" int vs_gemm_frame_loss(int compute, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* W, int64_t ldw,
                                  const float* bias, int act, const float* full, const int32_t* t_random_dev, int ae_shift, int first_forecast,
                                  int G, int T, const float* s_old, const float* s_new, int64_t n_s, const float* t0, int64_t Bt, int64_t Ct,
                                  int average_tloss, const float* lambdas, const float* grad_total, void* dz, int dz_dtype, float* ds_old,
                                  float* ds_new, float* dt0, float* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    VS_CHECK_ARG(compute == VS_BF16 || compute == VS_F16, "vs_gemm_frame_loss: 16-bit compute types only (%d)", compute);
    VS_CHECK_ARG(M > 0 && M < (1ll << 31) && N > 0 && K > 0 && G >= 1 && M % G == 0 && N % 4 == 0, "vs_gemm_frame_loss: bad sizes (rows = B * G, N %% 4 == 0)");
    VS_CHECK_ARG(!bias || ((uintptr_t)bias & 15) == 0, "vs_gemm_frame_loss: the bias must be 16-byte aligned");
    VS_CHECK_ARG(A && W && full && t_random_dev && grad_total && dz && dt0 && out && (n_s == 0 || (ds_old && ds_new)), "vs_gemm_frame_loss: null pointer");
    VS_CHECK_ARG(lda >= K && ldw >= K, "vs_gemm_frame_loss: leading dimension too small");
    VS_CHECK_ARG(vs_dtype_ok(dz_dtype) && act >= VS_ACT_NONE && act <= VS_ACT_ELU, "vs_gemm_frame_loss: bad dz dtype / activation");
    LossArgs a;
    int rc = fill_loss_args(a, nullptr, full, nullptr, t_random_dev, ae_shift, first_forecast, M / G, G, T, N, s_old, s_new, n_s, t0, Bt, Ct,
                            average_tloss, lambdas);
    if (rc != VS_OK) return rc;
    // its own acceptance, not plan_gemm's chain: the staggered tile in its 256 x 256 form, else the 256x256 tile, one split each
    const GemmPlan pp = p8_plan(compute, M, N, K, 1), bp = big_plan(compute, M, N, K, 1);
    auto takes = [&](const GemmPlan& p) {
        return p.use && dma_operands_ok(p.kind, A, lda, LR, 0, W, ldw, LR, 0, M, N, K) && p.splits == 1 && (int64_t)p.tiles_m * p.tiles_n <= VS_LOSS_MAX_PARTIALS;
    };
    const bool p8 = takes(pp) && pp.ni == 2;
    if (!p8 && !takes(bp)) return vs_fail(VS_ERR_UNSUPPORTED, "vs_gemm_frame_loss: the problem does not run on the 256x256 tile kernels");
    Epi epi = plain_epi(nullptr, N, VS_F32, 1.f);
    epi.bias = bias; epi.act = act;
    epi.fl_full = full; epi.fl_tdev = t_random_dev; epi.fl_ae_shift = ae_shift; epi.fl_first = first_forecast; epi.fl_G = G; epi.fl_T = T;
    epi.fl_up = grad_total; epi.fl_l_ae = a.l_ae; epi.fl_l_pred = a.l_pred; epi.fl_inv_ae = a.inv_ae; epi.fl_inv_pred = a.inv_pred;
    epi.fl_dz = dz; epi.fl_dz_dtype = dz_dtype; epi.fl_partials = out + 16;
    const GemmCall call{A, lda, LR, W, ldw, LR, M, N, K, 1, stream};
    rc = with_compute(compute, [&](auto ct) -> int {
        constexpr int CT = decltype(ct)::value;
        if (p8 && act == VS_ACT_SIGMOID) return launch_p8<CT, LR, LR, 2, 2>(call, pp, epi, nullptr);
        if (p8) return launch_p8<CT, LR, LR, 2, 1>(call, pp, epi, nullptr);
        return launch_big<CT, LR, LR, true>(call, bp, epi, nullptr);
    });
    if (rc != VS_OK) return rc;
    LossGrads gr{grad_total, dz, dz_dtype, act, ds_old, ds_new, dt0};
    hipLaunchKernelGGL(frame_loss_finish_kernel, dim3(1), dim3(256), 0, stream, a, out, p8 ? pp.tiles_m * pp.tiles_n : bp.tiles_m * bp.tiles_n, gr);
    VS_CHECK_LAUNCH("vs_gemm_frame_loss");
    return VS_OK;
}

extern "C" int vs_gemm(int compute, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, int layout_a, const void* B,
                       int64_t ldb, int layout_b, void* C, int64_t ldc, int c_dtype, float alpha, const float* bias, int act,
                       const void* mask, int64_t ldmask, int mask_dtype, int mask_act, int accumulate, void* workspace,
                       size_t workspace_bytes, void* stream_) {
    VS_CHECK_ARG(vs_dtype_ok(compute), "vs_gemm: compute type %d", compute);
    VS_CHECK_ARG(M > 0 && N > 0 && K > 0, "vs_gemm: M, N, K must be positive (%lld %lld %lld)", (long long)M, (long long)N, (long long)K);
    VS_CHECK_ARG(A && B && C, "vs_gemm: null operand");
    VS_CHECK_ARG((layout_a == LR || layout_a == LS) && (layout_b == LR || layout_b == LS), "vs_gemm: bad layout");
    VS_CHECK_ARG(vs_dtype_ok(c_dtype) && (!mask || vs_dtype_ok(mask_dtype)), "vs_gemm: bad c_dtype / mask_dtype");
    VS_CHECK_ARG(lda >= (layout_a == LR ? K : M) && ldb >= (layout_b == LR ? K : N) && ldc >= N, "vs_gemm: leading dimension too small");
    VS_CHECK_ARG(!mask || ldmask >= N, "vs_gemm: ldmask too small");
    VS_CHECK_ARG(act >= VS_ACT_NONE && act <= VS_ACT_ELU, "vs_gemm: bad activation");
    Epi epi = plain_epi(C, ldc, c_dtype, alpha);       // splits_per_batch = 0 and no batch strides: the single-problem form
    epi.bias = bias; epi.act = act;
    epi.mask = mask; epi.ldmask = ldmask; epi.mask_dtype = mask_dtype; epi.mask_act = mask_act;
    epi.accumulate = accumulate;
    const GemmPlan plan = plan_gemm(compute, M, N, K, 1, A, lda, layout_a, 0, B, ldb, layout_b, 0);
    const GemmCall call{A, lda, layout_a, B, ldb, layout_b, M, N, K, 1, (hipStream_t)stream_};
    return run_gemm("vs_gemm", compute, call, plan, epi, workspace, workspace_bytes);
}

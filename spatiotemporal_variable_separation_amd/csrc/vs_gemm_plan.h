// vs_gemm_plan.h -- which tile kernel runs a dense contraction, and in how many K splits.
//
// Five tile families serve vs_gemm / vs_gemm_batched (vs_gemm.hip): the register-staged tile (vs_gemm_core.h), the LDS-DMA 128x128 tile
// (vs_gemm_glds.h), the 128x128 ring tile (vs_gemm_mid.h), the 256x256 tile (vs_gemm_big.h) and the staggered 256-row tile (vs_gemm_p8.h).
// Every "when to take it" rule lives here: one candidate rule per family, the operand check of the LDS-DMA loaders, the priority chain
// (plan_gemm), the workspace bound (gemm_workspace_bytes) and the rule for finishing split-K inside the launch.  The headers above keep
// the kernels and their launchers.  Host code only: nothing here touches the runtime (vs_gemm_plan, the host-only ABI entry, prints it).
#pragma once
#include "vs_gemm_mid.h"
#include "vs_gemm_p8.h"

namespace {

enum { GEMM_REG = 0, GEMM_GLDS = 1, GEMM_MID = 2, GEMM_BIG = 3, GEMM_P8 = 4 };

// `use`: the family's rule takes the problem (a candidate; plan_gemm picks among them).  bm x bn: the output tile; tiles_m x tiles_n of them.
// k_tiles_per_split counts K tiles of the family's depth (64 / 16 fp32 register tile, BIG_BK ring and 256x256 tiles, P8_BK staggered tile).
// stages: ring tile only; ni, mi: staggered tile only (bn = 128 ni, bm = 64 mi).
struct GemmPlan {
    int kind; bool use;
    int bm, bn, splits; int64_t k_tiles_per_split;
    int tiles_m, tiles_n, stages, ni, mi;
};

// ---- register-staged tile (always applicable: the end of the chain, and the tile of the convolutions' implicit GEMMs) ---------------------
inline GemmPlan reg_plan(int compute, int64_t M, int64_t N, int64_t K, int64_t batch = 1) {
    const int bk = compute != VS_F32 ? 64 : 16;
    GemmPlan p{};
    p.kind = GEMM_REG;
    p.use = true;
    // Tile choice (measured on the config-2 shapes, tools/gemm_bench.py): the kernel keeps ~3 workgroups (12 waves) per CU
    // busy; with fewer than ~4 tiles of 128x128 per CU most SIMDs hold a single wave that cannot overlap its LDS reads with
    // MFMA and 128x64 wins (421 vs 312 TF/s at 3328x4096x1200); 64x64 wins when K is short (310 vs 172 TF/s at K = 256);
    // few-tile problems go to split-K, where larger tiles mean fewer fp32 slabs.
    const int64_t t128 = vs_cdiv(M, 128) * vs_cdiv(N, 128);
    const int64_t t12864 = vs_cdiv(M, 128) * vs_cdiv(N, 64);
    // 128x64 only from ~2.3 tiles per CU upwards.  Below that the step is faster with 64x64 tiles although the isolated kernel is
    // not (WaveEq B=128, whole recorded step: 1.51 -> 1.43 ms; 3328x1200 outputs are 494 tiles of 128x64 but 988 of 64x64, and
    // the 256x1200 encoder outputs 38 against 76): the launches overlap with the gradient branches, where more and lighter
    // workgroups fill the CUs the neighbours leave.
    constexpr int64_t t64_below = 600;
    if (const char* f = getenv("VS_GEMM_TILE")) {                       // debugging aid: force a tile ("128x128", "128x64", "64x64")
        p.bm = atoi(f); const char* x = strchr(f, 'x'); p.bn = x ? atoi(x + 1) : p.bm;
    } else if (K <= 512 && t128 >= 256) { p.bm = 64; p.bn = 64; }      // short K: prologue/epilogue bound, many small tiles win
    else if (t128 >= 1024) { p.bm = 128; p.bn = 128; }                 // >= 4 big tiles per CU: best LDS reuse
    else if ((t12864 >= 160 || vs_cdiv(M, 64) * vs_cdiv(N, 64) < 256) && M > 64 && t12864 >= t64_below) { p.bm = 128; p.bn = 64; }
    else { p.bm = 64; p.bn = 64; }
    if (M <= 64) p.bm = 64;
    if (N <= 64) p.bn = 64;
    if (p.bm == 64) p.bn = 64;
    // <= 64 output rows x very many columns (64-channel convolution layers over a whole batch of pixels): a 64x128 tile gives
    // every wave two accumulators per A fragment (1.5 LDS fragment reads per MFMA instead of 2)
    if (compute != VS_F32 && !getenv("VS_GEMM_TILE") && M <= 64 && M > 32 && vs_cdiv(N, 128) >= 1024 && K >= 128) { p.bm = 64; p.bn = 128; }
    p.tiles_m = (int)vs_cdiv(M, p.bm);
    p.tiles_n = (int)vs_cdiv(N, p.bn);
    const int64_t tiles = vs_cdiv(M, p.bm) * vs_cdiv(N, p.bn) * batch;
    const int64_t kt = vs_cdiv(K, bk);
    int splits = 1;
    if (tiles < 192 && kt >= 8) {
        splits = (int)((512 + tiles - 1) / tiles);
        const int64_t max_by_k = kt / 4;            // keep >= 4 K tiles per split
        if (splits > max_by_k) splits = (int)max_by_k;
        if (splits > 64) splits = 64;
        if (splits < 1) splits = 1;
    } else if (tiles < 1024 && kt >= 128) {
        // long reductions over few tiles (convolution weight gradients: K = batch x pixels up to ~10^6): one workgroup per CU
        // walking thousands of K tiles is latency bound; aim at ~1024 workgroups, >= 32 K tiles each
        splits = (int)((1024 + tiles - 1) / tiles);
        const int64_t max_by_k = kt / 32;
        if (splits > max_by_k) splits = (int)max_by_k;
        if (splits > 64) splits = 64;
        if (splits < 1) splits = 1;
    }
    p.k_tiles_per_split = vs_cdiv(kt, splits);
    p.splits = (int)vs_cdiv(kt, p.k_tiles_per_split);
    return p;
}

// ---- 256x256 tile ------------------------------------------------------------------------------------------------------------------------
// One workgroup per CU.  The plan asks for ONE round of 160..256 workgroups, >= 12 K tiles (of 32) (amortises prologue + epilogue:
// ~26 us of a 63 us launch at 3328 x 4096 x 1200 are launch, ring fill and the 54 MB of fp32 output), and enough work that the
// 256-wide tile is not mostly padding.  VS_GEMM_BIG=0 disables, =2 takes it whenever the operands allow (tests; split-K off).
// Measured (MI355X, bf16, random operands): 3328 x 4096 x 1200 63 us (128x64 tile:
// 76 us), 4096^3 158 us = 870 TFLOP/s (128x128 LDS-DMA tile: 184 us).  Timing-only variants of the loop: without
// the MFMAs and fragment reads the DMA ring alone runs at 0.57 us per 32 KiB tile (57 GB/s per CU), without real DMA traffic
// the multiply alone at 0.74 us per tile (MFMA-issue bound at the clock the chip holds under load), both together at 1.03 us.
inline GemmPlan big_plan(int compute, int64_t M, int64_t N, int64_t K, int64_t batch) {
    GemmPlan p{};
    p.kind = GEMM_BIG;
    p.bm = p.bn = 256;
    p.splits = 1;
    p.tiles_m = (int)vs_cdiv(M, 256);
    p.tiles_n = (int)vs_cdiv(N, 256);
    const char* env = getenv("VS_GEMM_BIG");                      // read per call: tests switch it
    const int mode = env ? atoi(env) : 1;
    if (compute == VS_F32 || mode == 0) return p;
    const int64_t kt = vs_cdiv(K, BIG_BK);
    const int64_t tiles = (int64_t)p.tiles_m * p.tiles_n * batch;
    p.k_tiles_per_split = kt;
    if (mode == 2) { p.use = tiles <= 65535; return p; }
    if (M < 512 || N < 512 || kt < 12 || tiles > 256) return p;
    // padding waste of the 256-wide tiles
    const double fill = (double)M * (double)N / ((double)p.tiles_m * 256.0 * (double)p.tiles_n * 256.0);
    if (fill < 0.8) return p;
    // Split-K is NOT planned: measured on the WaveEq decoder shapes the slab round trip of 256-wide tiles (4 B written + read per
    // output element and split) costs more than it buys -- 3328x1200x4096: 90 us split in 3 vs 78 us on the 128x64 tile,
    // 3328x1200x1200: 53 vs 35 us -- so the tile is taken where its tiles alone fill most of the chip (>= 160 of 256 CUs).
    if (tiles < 160) return p;
    p.use = true;
    return p;
}

// ---- 128x128 ring tile -------------------------------------------------------------------------------------------------------------------
// VS_GEMM_MID=0 disables, =2 takes it whenever the operands allow (tests).
inline GemmPlan mid_plan(int compute, int64_t M, int64_t N, int64_t K, int64_t batch) {
    GemmPlan p{};
    p.kind = GEMM_MID;
    p.bm = p.bn = 128;
    p.splits = 1;
    p.tiles_m = (int)vs_cdiv(M, 128);
    p.tiles_n = (int)vs_cdiv(N, 128);
    p.stages = 5;
    const char* env = getenv("VS_GEMM_MID");                      // read per call: tests switch it
    const int mode = env ? atoi(env) : 1;
    if (compute == VS_F32 || mode == 0) return p;
    const int64_t kt = vs_cdiv(K, BIG_BK);
    const int64_t tiles = (int64_t)p.tiles_m * p.tiles_n * batch;
    p.k_tiles_per_split = kt;
    if (mode == 2) { p.use = tiles <= 65535 * 4; p.stages = tiles <= 256 ? 10 : 5; return p; }
    if (M < 128 || N < 128 || kt < 16) return p;                   // short K: prologue / epilogue bound, the small tiles win
    const double fill = (double)M * (double)N / ((double)p.tiles_m * 128.0 * (double)p.tiles_n * 128.0);
    if (fill < 0.75) return p;
    // two workgroups per CU are resident: up to 512 in one round.  Few tiles and a long K: split so that ~one round is filled
    // and every split keeps >= 12 K tiles (prologue + epilogue + the slab round trip cost ~8 tiles' worth).
    int splits = 1;
    if (tiles < 200 && kt >= 24) {
        splits = (int)(448 / tiles);
        const int64_t max_by_k = kt / 12;
        if (splits > max_by_k) splits = (int)max_by_k;
        if (splits > 32) splits = 32;
        if (splits < 1) splits = 1;
    }
    // Taken where it wins INSIDE the WaveEq step, not only alone (same-box A/B of the replayed step): problems of 280..520
    // workgroups -- 4096 x 1200 x 3328 (320 tiles: 54 vs 81 us alone, 70 vs 140 us under the integrator's backward kernel),
    // 1200 x 1200 x 3328 split in 4, 256 x 1200 x 20480 split in 22.  At 260 workgroups (3328 x 1200 x K: one per CU) it is
    // 33.8 vs 35.3 us alone but 54 vs 45 us in the step, where its 80 KiB of LDS per workgroup keeps neighbours off the CU.
    if (tiles * splits < 280 || tiles * splits > 520) return p;
    p.k_tiles_per_split = vs_cdiv(kt, splits);
    p.splits = (int)vs_cdiv(kt, p.k_tiles_per_split);
    p.stages = tiles * p.splits <= 256 ? 10 : 5;
    p.use = true;
    return p;
}

// the ring tile as vs_gemm_adam launches it: one split whatever K (the optimizer epilogue needs the whole sum), 5 stages
inline GemmPlan ring_plan_one_split(int64_t M, int64_t N, int64_t K) {
    GemmPlan p{};
    p.kind = GEMM_MID;
    p.use = true;
    p.bm = p.bn = 128;
    p.splits = 1;
    p.k_tiles_per_split = vs_cdiv(K, BIG_BK);
    p.tiles_m = (int)vs_cdiv(M, 128);
    p.tiles_n = (int)vs_cdiv(N, 128);
    p.stages = 5;
    return p;
}

// ---- staggered 256-row tile --------------------------------------------------------------------------------------------------------------
// One workgroup per CU (128 / 96 KiB of LDS).  VS_GEMM_P8: 0 = never, 1 = by plan (default), 2 = whenever the operands allow (tests).
inline GemmPlan p8_plan(int compute, int64_t M, int64_t N, int64_t K, int64_t batch) {
    GemmPlan p{};
    p.kind = GEMM_P8;
    p.splits = 1;
    p.k_tiles_per_split = vs_cdiv(K, P8_BK);
    auto tile = [&](int ni, int mi) {                             // 256 x 256 (2, 4), 256 x 128 (1, 4) or 128 x 128 (1, 2)
        p.ni = ni; p.mi = mi; p.bm = 64 * mi; p.bn = 128 * ni;
        p.tiles_m = (int)vs_cdiv(M, p.bm); p.tiles_n = (int)vs_cdiv(N, p.bn);
    };
    tile(2, 4);
    const char* env = getenv("VS_GEMM_P8");                       // read per call: tests switch it
    const int mode = env ? atoi(env) : 1;
    if (compute == VS_F32 || mode == 0) return p;
    const char* env_ni = getenv("VS_GEMM_P8_NI");
    const int force_ni = env_ni ? atoi(env_ni) : 0;
    auto fill_of = [&](int bn) { return (double)M * (double)N / ((double)vs_cdiv(M, 256) * 256.0 * (double)vs_cdiv(N, bn) * (double)bn); };
    const char* env_mi = getenv("VS_GEMM_P8_MI");
    const int force_mi = env_mi ? atoi(env_mi) : 0;
    if (mode == 2) {
        if (force_ni == 1) tile(1, force_mi == 2 ? 2 : 4);
        p.use = (int64_t)p.tiles_m * p.tiles_n * batch <= 65535;
        return p;
    }
    // One tile row, long K (the encoders' first layer, 256 x 1200 x 20480: the weight matrix is streamed once, HBM-bound): 256 x 128 tiles, K split
    // over ~one round of CUs into fp32 slabs (reduced by splitk_reduce_kernel).  Measured against the 128 x 128 ring tile (20 tiles x 22 splits):
    // alone, cold operands 43.5 -> 38.1 us; replayed WaveEq step, two interleaved pairs 1.2414 / 1.2337 -> 1.2114 / 1.2079 ms.
    {
        const int64_t kt = p.k_tiles_per_split, tn = vs_cdiv(N, 128);
        if (M > 128 && M <= 256 && N >= 512 && kt >= 64 && tn * batch <= 64 && (double)N / (tn * 128.0) >= 0.85) {
            int64_t splits = 250 / (tn * batch);
            if (splits > kt / 8) splits = kt / 8;
            if (splits >= 2) {
                tile(1, 4);
                p.k_tiles_per_split = vs_cdiv(kt, splits);
                p.splits = (int)vs_cdiv(kt, p.k_tiles_per_split);
                p.use = true;
                return p;
            }
        }
    }
    if (M < 512 || N < 512 || p.k_tiles_per_split < 6) return p;
    const int64_t t256 = (int64_t)p.tiles_m * p.tiles_n * batch;
    if (t256 >= 160 && fill_of(256) >= 0.8) { p.use = true; return p; }
    // 256 x 128 where the 256-wide tiles leave most CUs idle (decoder layers of the WaveEq model, 3328 x 1200: 65 -> 130 tiles; measured in the
    // replayed WaveEq step against the 64 x 64 tile, two interleaved pairs: 1.2309 / 1.2380 vs 1.2424 / 1.2459 ms).  VS_GEMM_P8_NI=2: never.
    // 128 x 128 (MI = 2, two workgroups per CU) where that fills the chip once: 3328 x 1200 -> 260 workgroups on 512 slots.  VS_GEMM_P8_MI=4: never.
    const int64_t t128sq = (int64_t)vs_cdiv(M, 128) * vs_cdiv(N, 128) * batch;
    const double fill128sq = (double)M * (double)N / ((double)vs_cdiv(M, 128) * 128.0 * (double)vs_cdiv(N, 128) * 128.0);
    if (force_ni != 2 && force_mi != 4 && force_mi == 2 && t128sq >= 200 && t128sq <= 512 && fill128sq >= 0.85 && p.k_tiles_per_split >= 8) {
        tile(1, 2);
        p.use = true;
        return p;
    }
    const int64_t t128 = (int64_t)p.tiles_m * vs_cdiv(N, 128) * batch;
    if (force_ni != 2 && t128 >= 96 && t128 <= 256 && fill_of(128) >= 0.85 && p.k_tiles_per_split >= 8) {
        tile(1, 4);
        p.use = true;
    }
    return p;
}

// ---- which family runs a call -------------------------------------------------------------------------------------------------------------
// Both operands fit the family's LDS-DMA loader (16-byte alignment, multiples of 8) and its 32-bit lane offsets inside a tile
inline bool dma_operands_ok(int kind, const void* A, int64_t lda, int la, int64_t stride_a, const void* B, int64_t ldb, int lb, int64_t stride_b,
                            int64_t M, int64_t N, int64_t K) {
    const int64_t ld_limit = kind == GEMM_GLDS ? INT64_MAX : kind == GEMM_MID ? 1ll << 23 : 1ll << 22;
    return glds_operand_ok(A, lda, la, M, K, stride_a) && glds_operand_ok(B, ldb, lb, N, K, stride_b) && lda < ld_limit && ldb < ld_limit;
}

// Priority: staggered tile, 256x256 tile, ring tile, register tile; a family whose loader the operands do not fit falls through to the next.
inline GemmPlan plan_gemm(int compute, int64_t M, int64_t N, int64_t K, int64_t batch, const void* A, int64_t lda, int la, int64_t stride_a,
                          const void* B, int64_t ldb, int lb, int64_t stride_b) {
    auto fits = [&](int kind) { return dma_operands_ok(kind, A, lda, la, stride_a, B, ldb, lb, stride_b, M, N, K); };
    for (const GemmPlan& p : {p8_plan(compute, M, N, K, batch), big_plan(compute, M, N, K, batch), mid_plan(compute, M, N, K, batch)})
        if (p.use && fits(p.kind)) return p;
    GemmPlan p = reg_plan(compute, M, N, K, batch);
    // LDS-DMA staged tile (vs_gemm_glds.h) wherever the register rule picks 128x128 (>= 1024 tiles).  Measured on MI355X
    // (tools/gemm_bench.py): 732 vs 588 TF/s at 4096^3 with two LDS buffers; with S operands it is not faster than the
    // register-staged tile yet (598 vs 593), so only R x R takes this path.  At 512-1023 tiles (the decoder's
    // 3328x4096x1200: 832 tiles on 768 / 512 resident slots) 128x64 register staging stays ahead: 75 vs 89-98 us.
    // VS_GEMM_GLDS=0 disables, =2 forces all layouts.
    static const int glds_mode = getenv("VS_GEMM_GLDS") ? atoi(getenv("VS_GEMM_GLDS")) : 1;
    if (compute != VS_F32 && p.bm == 128 && p.bn == 128 && (la == LR && lb == LR ? glds_mode != 0 : glds_mode == 2) && fits(GEMM_GLDS))
        p.kind = GEMM_GLDS;
    return p;
}

// ---- split-K slabs ------------------------------------------------------------------------------------------------------------------------
inline size_t gemm_slab_bytes(const GemmPlan& p, int64_t M, int64_t N, int64_t batch) {
    return p.splits > 1 ? (size_t)batch * p.splits * (size_t)M * (size_t)N * sizeof(float) : 0;
}

// Upper bound of the slab area of any call with these sizes: the worst over the compute types and over EVERY family whose rule takes the
// problem, whatever the operands look like (a misaligned operand falls through to a lower family).
inline size_t gemm_workspace_bytes(int64_t M, int64_t N, int64_t K, int64_t batch) {
    if (batch <= 0 || M <= 0 || N <= 0 || K <= 0) return 0;
    size_t worst = 0;
    for (int c = 0; c < 2; ++c)                        // fp32 and the 16-bit types (bf16 and fp16 plan alike)
        for (const GemmPlan& p : {reg_plan(c, M, N, K, batch), big_plan(c, M, N, K, batch), mid_plan(c, M, N, K, batch), p8_plan(c, M, N, K, batch)})
            if (p.use && gemm_slab_bytes(p, M, N, batch) > worst) worst = gemm_slab_bytes(p, M, N, batch);
    return worst;
}

// Split-K may be finished inside the launch (arrival counters, vs_gemm.hip) on the register tile except 128x128 and on the ring tile (the
// 128x128 LDS-DMA tile never splits in practice, the 256-row tiles have no fix-up); one counter per (problem, tile), and the last workgroup
// of a tile reads back splits x tile x 4 bytes.  The kernels address the slab area with 32-bit offsets: no counters (0) from 2 GiB upwards.
inline bool gemm_splitk_in_launch(const GemmPlan& p) {
    return p.splits > 1 && (p.kind == GEMM_MID || (p.kind == GEMM_REG && !(p.bm == 128 && p.bn == 128)));
}
inline int64_t gemm_splitk_counters(const GemmPlan& p, int64_t M, int64_t N, int64_t batch) {
    return gemm_slab_bytes(p, M, N, batch) < (1ull << 31) ? batch * p.tiles_m * p.tiles_n : 0;
}
inline int64_t gemm_splitk_tile_bytes(const GemmPlan& p) { return (int64_t)p.splits * p.bm * p.bn * 4; }

}  // namespace

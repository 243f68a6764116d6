// vs_mt19937_core.h -- the logic of vs_mt19937_randint (csrc/vs_mt19937.hip) as plain __host__ __device__ functions: NumPy's legacy stream
// (np.random.RandomState: MT19937) and its scalar `randint(low, high)`, drawn as a table.  The header compiles with a host compiler alone
// (tests/host/mt19937_host_check.cpp), so the logic runs on the CPU, under sanitizers, before it runs on a GPU, and the kernel's words are
// the host's words: one logic, two builds.
//
// The stream.  State: key[624] and pos.  While pos >= 624 the block is regenerated (the standard twist: M = 397, matrix 0x9908b0df) and pos
// becomes 0; the output is key[pos++], tempered.  randint(low, high): rng = high - 1 - low (as a 32-bit unsigned number; int32 bounds give
// rng <= 2^32 - 2).  rng == 0: the result is low and NO output is consumed.  Otherwise mask = rng with every bit below its top bit set,
// v = next32 & mask is repeated until v <= rng, and the result is low + v.  A block is regenerated only when an output of it is needed: a
// call that ends exactly on pos == 624 leaves the old key in place.  NumPy takes this 32-bit path for every rng an int32 pair can give;
// the wide ranges (-2^31, 2^31 - 1) and (0, 2^31 - 1) are among the cases compared with it (tests/mmnist_draws_inputs.py), so nothing is
// refused for its width.
//
// What one call makes: out[r, j], r < n_rows, j < k <= 8, is the (r * k + j)-th scalar randint(low[j], high[j]) of the stream; the state is
// advanced past the output that completed the last draw.  With every column at rng == 0 the state is not touched.
//
// Execution model: `nlanes` lanes (host: 1, or the lanes of the test's emulation; device: the 256 of one workgroup) work on a WINDOW of at
// most nlanes consecutive outputs of the current block, lane i on output pos + i.  Which draw takes which output is decided by the column
// that is waiting, so every output defines a map on the k' <= 8 waiting states (k': the columns that consume): s -> s + 1 (mod k') when
// (out & mask[s]) <= rng[s], s otherwise.  Maps compose associatively; an exclusive scan of the packed maps (4 bits per state in one
// 32-bit word) gives every output the state it meets, a prefix sum of the accepted outputs gives each its draw index d, hence its place
// (d / k', column of state d % k').  The lane primitives are macros with host defaults for one lane: VSM_SYNC (barrier), VSM_SCAN_MAP
// (exclusive scan under vsm_compose and the composition of all lanes), VSM_SCAN_ADD (exclusive prefix sum and sum).  No decision depends on
// nlanes: the windows only cut the same sequence of outputs at other places.
//
// Termination and bounds, on ANY state:
//   * a window holds 1 .. 624 - pos outputs, so key[] is read inside its 624 words; regeneration reads old[i], old[i + 1], old/new[i +- 397]
//     with i < 624 spelled out per phase;
//   * a draw index at or above n_rows * k' is never written, so out[] is written inside its n_rows * k entries;
//   * every window consumes at least one output; the call gives up with VSM_STATUS_BUDGET once it has consumed 64 outputs per draw owed
//     plus 4096 without completing the draws (every column accepts an output with probability above 1/2, so this needs a run of some
//     thousand rejections: it guards a shared device against a state that is not a stream, not against a stream);
//   * pos > 624 is refused (VSM_STATUS_POS) before anything is written.
#pragma once
#include <stdint.h>

#ifndef VSM_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define VSM_HD __host__ __device__ inline
#else
#define VSM_HD inline
#endif
#endif
#ifndef VSM_PURE                                    /* no lane primitive inside: the entry point's host side calls these too */
#if defined(__HIPCC__) || defined(__CUDACC__)
#define VSM_PURE __host__ __device__ inline
#else
#define VSM_PURE inline
#endif
#endif
#ifndef VSM_SYNC
#define VSM_SYNC() ((void)0)
#define VSM_SCAN_MAP(m, before, total) ((before) = VSM_IDENTITY, (total) = (m))
#define VSM_SCAN_ADD(v, before, total) ((before) = 0, (total) = (v))
#endif

#define VSM_N 624
#define VSM_M 397
#define VSM_STATE_WORDS 625                         /* key[624], pos */
#define VSM_MAX_COLS 8
#define VSM_IDENTITY 0x76543210u                    /* the packed map s -> s */
#define VSM_STATUS_OK 0
#define VSM_STATUS_POS 1                            /* pos > 624 read from the state: nothing was written */
#define VSM_STATUS_BUDGET 2                         /* the outputs' budget ran out: out[] is partly written, the state is not advanced */

// the columns of a table, prepared once per call (on the host, by value into the kernel)
struct VsmCols {
    int32_t k, kact;                                // columns; columns with rng != 0, the ones that consume outputs
    int32_t low[VSM_MAX_COLS];
    uint32_t rng[VSM_MAX_COLS], mask[VSM_MAX_COLS]; // by column
    int32_t act[VSM_MAX_COLS];                      // waiting state s -> its column
};

// the scratch the lanes share (LDS on the device)
struct VsmWork {
    uint32_t key[2][VSM_N];                         // the block and the block being made; `cur` names the live one
    int32_t end_pos;
};

VSM_PURE uint32_t vsm_mask_of(uint32_t rng) {
    uint32_t m = rng;
    m |= m >> 1; m |= m >> 2; m |= m >> 4; m |= m >> 8; m |= m >> 16;
    return m;
}

// lows[j] < highs[j] for every j < k, 1 <= k <= VSM_MAX_COLS (the caller has checked)
VSM_PURE void vsm_cols_init(VsmCols* c, const int32_t* lows, const int32_t* highs, int k) {
    c->k = k;
    c->kact = 0;
    for (int j = 0; j < VSM_MAX_COLS; ++j) {
        c->low[j] = j < k ? lows[j] : 0;
        c->rng[j] = j < k ? (uint32_t)highs[j] - 1u - (uint32_t)lows[j] : 0u;
        c->mask[j] = vsm_mask_of(c->rng[j]);
        c->act[j] = 0;
    }
    for (int j = 0; j < k; ++j)
        if (c->rng[j] != 0u) c->act[c->kact++] = j;
}

VSM_HD uint32_t vsm_temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

VSM_HD uint32_t vsm_twist(uint32_t u, uint32_t v) {
    const uint32_t y = (u & 0x80000000u) | (v & 0x7fffffffu);
    return (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

// The next block from `old` into `nw` (two different arrays of 624 words), in three phases: new[i] needs old[i], old[i + 1] and word
// i + 397 of the block, which is an old word for i < 227 and the new word i - 227, written one phase earlier, from there on.
VSM_HD void vsm_regenerate(const uint32_t* old, uint32_t* nw, int lane, int nlanes) {
    VSM_SYNC();                                     // nobody still reads nw[] as the block before this one
    for (int i = lane; i < VSM_N - VSM_M; i += nlanes) nw[i] = old[i + VSM_M] ^ vsm_twist(old[i], old[i + 1]);
    VSM_SYNC();
    for (int i = VSM_N - VSM_M + lane; i < 2 * (VSM_N - VSM_M); i += nlanes) nw[i] = nw[i - (VSM_N - VSM_M)] ^ vsm_twist(old[i], old[i + 1]);
    VSM_SYNC();
    for (int i = 2 * (VSM_N - VSM_M) + lane; i < VSM_N; i += nlanes)       // 454 .. 623; the last word wraps to new[0]
        nw[i] = nw[i - (VSM_N - VSM_M)] ^ vsm_twist(old[i], i + 1 < VSM_N ? old[i + 1] : nw[0]);
    VSM_SYNC();
}

// does the column with (rng, mask) accept the output y?  v: the masked value, low + v the result
VSM_HD bool vsm_bounded(uint32_t y, uint32_t rng, uint32_t mask, uint32_t* v) {
    *v = y & mask;
    return *v <= rng;
}

// the packed map of one output on the waiting states 0 .. kact - 1 (states above stay where they are)
VSM_HD uint32_t vsm_map_of(const VsmCols* c, uint32_t y) {
    uint32_t m = VSM_IDENTITY, v;
    for (int s = 0; s < c->kact; ++s) {
        const int j = c->act[s];
        if (vsm_bounded(y, c->rng[j], c->mask[j], &v)) {
            const uint32_t to = s + 1 == c->kact ? 0u : (uint32_t)s + 1u;
            m = (m & ~(0xFu << (4 * s))) | (to << (4 * s));
        }
    }
    return m;
}
VSM_HD uint32_t vsm_apply(uint32_t map, uint32_t s) { return (map >> (4 * s)) & 7u; }
// first `a`, then `b`
VSM_HD uint32_t vsm_compose(uint32_t a, uint32_t b) {
    uint32_t c = 0;
    for (int s = 0; s < VSM_MAX_COLS; ++s) c |= vsm_apply(b, vsm_apply(a, (uint32_t)s)) << (4 * s);
    return c;
}

// The table.  state: 625 words, read by every lane and written back at the end; out: n_rows * c->k entries.  Every lane calls it with the
// same arguments; the return value (a VSM_STATUS_*) is the same on every lane.
VSM_HD int vsm_fill_table(uint32_t* state, VsmWork* w, const VsmCols* c, int64_t n_rows, int32_t* out, int lane, int nlanes) {
    uint32_t pos = state[VSM_N];
    if (pos > VSM_N) return VSM_STATUS_POS;
    const int k = c->k, kact = c->kact;
    for (int64_t i = lane; i < n_rows * k; i += nlanes) {                  // the columns that consume nothing
        const int j = (int)(i % k);
        if (c->rng[j] == 0u) out[i] = c->low[j];
    }
    const int64_t owed = n_rows * kact;
    if (owed == 0) return VSM_STATUS_OK;
    for (int i = lane; i < VSM_N; i += nlanes) w->key[0][i] = state[i];
    VSM_SYNC();
    int cur = 0;
    int64_t done = 0, budget = 64 * owed + 4096;
    uint32_t s0 = 0;                                                       // the state that waits at the window's first output
    while (done < owed) {
        if (budget <= 0) return VSM_STATUS_BUDGET;
        if (pos >= VSM_N) {
            vsm_regenerate(w->key[cur], w->key[cur ^ 1], lane, nlanes);
            cur ^= 1;
            pos = 0;
        }
        const int width = (int)(VSM_N - pos) < nlanes ? (int)(VSM_N - pos) : nlanes;
        const bool live = lane < width;
        const uint32_t y = live ? vsm_temper(w->key[cur][pos + lane]) : 0u;
        const uint32_t m = live ? vsm_map_of(c, y) : VSM_IDENTITY;
        uint32_t before, all;
        VSM_SCAN_MAP(m, before, all);
        const uint32_t s = vsm_apply(before, s0);
        const int j = c->act[s];
        uint32_t v;
        const bool taken = vsm_bounded(y, c->rng[j], c->mask[j], &v) && live;
        int ahead, total;
        VSM_SCAN_ADD(taken ? 1 : 0, ahead, total);
        const int64_t d = done + ahead;
        if (taken && d < owed) {
            out[(d / kact) * k + j] = (int32_t)((uint32_t)c->low[j] + v);
            if (d == owed - 1) w->end_pos = (int32_t)pos + lane + 1;       // one past the output that completed the last draw
        }
        VSM_SYNC();
        if (done + total >= owed) {
            pos = (uint32_t)w->end_pos;
            done = owed;
        } else {
            pos += (uint32_t)width;
            done += total;
            budget -= width;
            s0 = vsm_apply(all, s0);
        }
    }
    VSM_SYNC();
    for (int i = lane; i < VSM_N; i += nlanes) state[i] = w->key[cur][i];
    if (lane == 0) state[VSM_N] = pos;
    return VSM_STATUS_OK;
}

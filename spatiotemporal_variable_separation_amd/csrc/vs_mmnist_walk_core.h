// vs_mmnist_walk_core.h -- the logic of vs_mmnist_stochastic_trajectories (csrc/vs_mmnist_walk.hip) as plain __host__ __device__ functions:
// the STOCHASTIC Moving-MNIST sampler of the reference (data/moving_mnist.py:131-253 with deterministic=False), which redraws the speed
// vector from the NumPy stream inside the bounce loop, so that how many outputs a trajectory takes depends on the trajectory.  The stream
// is vs_mt19937_core.h's (twist, tempering, masked rejection); this header adds the walk.  It compiles with a host compiler alone
// (tests/host/mmnist_walk_host_check.cpp): one logic, two builds.
//
// One trajectory: n_pre scalar draws randint(low[j], high[j]) (training: digit index, start row, start column, row speed, column speed;
// n_pre == 4: the last four alone; n_pre < 4: the start state is row i of a caller's table int32 [n_traj, 4]), then seq_len steps: the
// collision passes, record (rint(sx), rint(sy), dx, dy), sy += dy, sx += dx.  The walker -- body, collision pass, record, move -- is
// vs_mmnist_bounce_core.h, which the deterministic sampler of csrc/vs_data.hip shares; this sampler's passes draw dx = randint(-max_speed,
// max_speed + 1), then dy likewise, between computing p and mirroring the speed (VswRedraw).  Passes and steps share one loop
// (vsw_trajectory).  A draw with high - 1 - low == 0 consumes nothing.
//
// Two forms over the same `vsw_trajectory`:
//   * vsw_walk_serial -- ONE lane walks the trajectories one after the other.  The host's default build and the checker of the other.
//   * vsw_walk_lanes  -- trajectory i + 1 starts where trajectory i stopped consuming, a chain through the stream; the lanes break it by
//     speculating on entry points.  WINDOW: the raw words of VSW_BLOCKS consecutive blocks (the state's key and the blocks after it, which
//     need only that key).  PASS 1: for every offset o from the current position to the window's end a lane walks a trajectory from o
//     without storing it and leaves jump[o] = where it stopped, VSW_PAST (it needs outputs beyond the window) or VSW_DEAD (bounce budget).
//     CHASE: starts[0] = pos, starts[i + 2^k] = jump^(2^k)[starts[i]] while jump is squared in place of its twin (pointer doubling, one
//     barrier per k).  PASS 2: lane i walks again from starts[i] and stores its rows.  ADVANCE: the window slides to the block that holds
//     the last output consumed, the blocks behind it are regenerated, and the round repeats until n_traj are done.  A trajectory that does
//     not fit a whole window (more than 1872 outputs) is walked by lane 0 with the serial reader, which slides the window alone.  The start
//     table form (n_pre < 4) makes the walk depend on i as well as on o, so it is walked by lane 0 throughout.
//   No decision depends on nlanes.
//
// Termination and bounds, on ANY state: pos > 624 is refused (VSM_STATUS_POS) before anything is written; the bounce loop gives up after
// VSW_MAX_PASSES passes per call (VSW_STATUS_BOUNCE); a draw gives up after VSW_DRAW_TRIES rejected outputs (VSM_STATUS_BUDGET; every
// column accepts with probability above 1/2); a speculative walk reads raw[o] with o < VSW_WINDOW only.  Rows are stored for t < seq_len,
// i < n_traj only.  On every non-zero status the state is not advanced (outputs may be partly written, except for VSM_STATUS_POS).
#pragma once
#include "vs_mmnist_bounce_core.h"
#include "vs_mt19937_core.h"

#define VSW_STATUS_BOUNCE 3                         /* a collision pass count above VSW_MAX_PASSES: the state is not advanced */
#define VSW_DRAW_TRIES 4096
#define VSW_BLOCKS 4
#define VSW_WINDOW (VSW_BLOCKS * VSM_N)             /* 2496 outputs */
#define VSW_PAST (VSW_WINDOW + 1)                   /* jump values beyond the offsets 0 .. VSW_WINDOW; both are fixed points */
#define VSW_DEAD (VSW_WINDOW + 2)
#define VSW_TABLE (VSW_WINDOW + 3)
#define VSW_ROUND 256                               /* trajectories resolved per round (2^8: eight doublings) */
#define VSW_RC_PAST (-1)                            /* vsw_trajectory: the window ended (speculative reader only) */

struct VswGeom {
    int32_t n_pre, seq_len, x_max, y_max;           // x: rows, y: columns, as in the reference
    int32_t speed_low;
    uint32_t speed_rng, speed_mask;
    VsmCols pre;                                    // the prefix columns (k == n_pre; unused when n_pre == 0)
};

// the scratch the lanes share (LDS on the device): 21 KiB
struct VswWork {
    uint32_t raw[VSW_WINDOW];                       // untempered words of VSW_BLOCKS consecutive blocks; block 0 is the state's key
    uint16_t jump[2][VSW_TABLE];
    int32_t starts[VSW_ROUND + 1];
    int32_t pos, made, status;                      // written by one lane between barriers, read by all
};

// the stream as a trajectory reads it: offset o into the window; the serial reader (one lane owns the window) slides it when it ends
struct VswReader {
    uint32_t* raw;
    int32_t o, serial;
};

// lows[j] < highs[j] for j < n_pre, 0 <= n_pre <= 5, max_speed >= 0 (the caller has checked)
VSM_PURE void vsw_geom_init(VswGeom* g, int n_pre, int seq_len, const int32_t* lows, const int32_t* highs, int x_max, int y_max, int max_speed) {
    g->n_pre = n_pre; g->seq_len = seq_len; g->x_max = x_max; g->y_max = y_max;
    g->speed_low = -max_speed;
    g->speed_rng = 2u * (uint32_t)max_speed;
    g->speed_mask = vsm_mask_of(g->speed_rng);
    int32_t none = 0, one = 1;
    vsm_cols_init(&g->pre, n_pre > 0 ? lows : &none, n_pre > 0 ? highs : &one, n_pre > 0 ? n_pre : 1);
}

// the block after `old` into `nw` by one lane alone (no barrier inside): vsm_regenerate's three phases in one loop
VSM_HD void vsw_regenerate_alone(const uint32_t* old, uint32_t* nw) {
    for (int i = 0; i < VSM_N; ++i) {
        const uint32_t far = i < VSM_N - VSM_M ? old[i + VSM_M] : nw[i - (VSM_N - VSM_M)];
        nw[i] = far ^ vsm_twist(old[i], i + 1 < VSM_N ? old[i + 1] : nw[0]);
    }
}

// blocks 1 .. VSW_BLOCKS - 1 of the window from block 0, by all lanes
VSM_HD void vsw_fill_window(uint32_t* raw, int from_block, int lane, int nlanes) {
    for (int b = from_block; b < VSW_BLOCKS; ++b) vsm_regenerate(raw + (b - 1) * VSM_N, raw + b * VSM_N, lane, nlanes);
}

// block `by` becomes block 0 (by >= 1) and the rest is made again, by all lanes
VSM_HD void vsw_slide(uint32_t* raw, int by, int lane, int nlanes) {
    VSM_SYNC();
    for (int b = 0; b + by < VSW_BLOCKS; ++b) {
        for (int i = lane; i < VSM_N; i += nlanes) raw[b * VSM_N + i] = raw[(b + by) * VSM_N + i];
        VSM_SYNC();                                 // block b + by is the target of a later turn
    }
    vsw_fill_window(raw, VSW_BLOCKS - by, lane, nlanes);
}

// one scalar randint from the reader: 0, VSW_RC_PAST or VSM_STATUS_BUDGET
VSM_HD int vsw_draw(VswReader* r, uint32_t rng, uint32_t mask, int32_t low, int32_t* out) {
    if (rng == 0u) { *out = low; return 0; }
    for (int tries = 0; tries < VSW_DRAW_TRIES; ++tries) {
        if (r->o >= VSW_WINDOW) {
            if (!r->serial) return VSW_RC_PAST;
            for (int i = 0; i < VSM_N; ++i) r->raw[i] = r->raw[(VSW_BLOCKS - 1) * VSM_N + i];       // the block of the last output stays: block 0
            for (int b = 1; b < VSW_BLOCKS; ++b) vsw_regenerate_alone(r->raw + (b - 1) * VSM_N, r->raw + b * VSM_N);
            r->o -= (VSW_BLOCKS - 1) * VSM_N;
        }
        uint32_t v;
        if (vsm_bounded(vsm_temper(r->raw[r->o++]), rng, mask, &v)) { *out = (int32_t)((uint32_t)low + v); return 0; }
    }
    return VSM_STATUS_BUDGET;
}

// The two redraws of a collision pass, dx then dy (the same column twice).  The serial reader draws them one by one.  A speculative walk
// is a chain of dependent window reads, and its lanes wait for the slowest rejection loop among them, so there EIGHT outputs are read at
// once (independent reads, one round trip): the first two accepted are dx and dy and the stream stands past the second -- the same
// outputs, taken by the same draws.  Fewer than two among the eight (1.5 % at max_speed 4): the next eight.
VSM_HD int vsw_draw_speeds(VswReader* r, const VswGeom* g, int32_t* pdx, int32_t* pdy) {
    const uint32_t rng = g->speed_rng, mask = g->speed_mask;
    if (rng == 0u) { *pdx = g->speed_low; *pdy = g->speed_low; return 0; }
    if (r->serial) {
        const int rc = vsw_draw(r, rng, mask, g->speed_low, pdx);
        return rc != 0 ? rc : vsw_draw(r, rng, mask, g->speed_low, pdy);
    }
    int found = 0;
    while (found < 2) {
        const int32_t o = r->o;
        if (o >= VSW_WINDOW) return VSW_RC_PAST;
        const int avail = VSW_WINDOW - o < 8 ? VSW_WINDOW - o : 8;
        uint32_t v[8];
#if defined(__clang__)
#pragma unroll
#endif
        for (int k = 0; k < 8; ++k) v[k] = vsm_temper(r->raw[o + (k < avail ? k : 0)]) & mask;   // never past the window
        int used = avail;
#if defined(__clang__)
#pragma unroll
#endif
        for (int k = 0; k < 8; ++k) {
            if (k < avail && found < 2 && v[k] <= rng) {
                const int32_t speed = (int32_t)((uint32_t)g->speed_low + v[k]);
                if (found == 0) *pdx = speed; else { *pdy = speed; used = k + 1; }
                ++found;
            }
        }
        r->o = o + used;
    }
    return 0;
}

// what a collision pass of this sampler does between computing p and mirroring the speed (vs_mmnist_bounce_core.h)
struct VswRedraw {
    VswReader* r;
    const VswGeom* g;
    VSM_HD int operator()(int32_t* pdx, int32_t* pdy) const { return vsw_draw_speeds(r, g, pdx, pdy); }
};

// Trajectory i from the reader.  With store != 0 its rows go to pre [n_traj, n_pre], positions [seq_len, n_traj, 2], latents [seq_len,
// n_traj, 4] (may be null) and desc [n_traj / nd, 1 + nd] (may be null; n_pre == 5).  start: int32 [n_traj, 4], read when n_pre < 4.
VSM_HD int vsw_trajectory(const VswGeom* g, VswReader* r, int64_t i, int64_t n_traj, const int32_t* start, int store, int32_t* pre,
                          int32_t* positions, int32_t* latents, int32_t* desc, int nd) {
    int32_t q[5] = {0, 0, 0, 0, 0};                 // constant indices only: registers, not scratch
#if defined(__clang__)
#pragma unroll
#endif
    for (int j = 0; j < 5; ++j) {
        if (j < g->n_pre) {
            const int rc = vsw_draw(r, g->pre.rng[j], g->pre.mask[j], g->pre.low[j], &q[j]);
            if (rc != 0) return rc;
        }
    }
    if (store) {
#if defined(__clang__)
#pragma unroll
#endif
        for (int j = 0; j < 5; ++j)
            if (j < g->n_pre) pre[i * g->n_pre + j] = q[j];
        if (desc) {
            const int64_t v = i / nd;
            if (i - v * nd == 0) desc[v * (1 + nd)] = (int32_t)v;
            desc[v * (1 + nd) + 1 + (i - v * nd)] = q[0];
        }
    }
    const bool five = g->n_pre == 5, table = g->n_pre < 4;
    const double sx = (double)(table ? start[i * 4] : five ? q[1] : q[0]), sy = (double)(table ? start[i * 4 + 1] : five ? q[2] : q[1]);
    const int32_t dx = table ? start[i * 4 + 2] : five ? q[3] : q[2], dy = table ? start[i * 4 + 3] : five ? q[4] : q[3];
    // One loop over passes AND steps: a turn is one collision pass while an edge is hit, else record and move.  Lanes of a wave that are at
    // different steps or passes of their trajectories share the turns instead of waiting for the longest collision of every step.
    VswBody s = vsw_body(g->x_max, g->y_max, sx, sy, dx, dy);
    const VswRedraw redraw = {r, g};
    for (int t = 0; t < g->seq_len;) {
        if (s.left || s.right || s.upper || s.bottom) {
            if (s.passes >= VSW_MAX_PASSES) return VSW_STATUS_BOUNCE;
            const int rc = vsw_pass(g->x_max, g->y_max, &s, redraw);
            if (rc != 0) return rc;
            continue;
        }
        if (store) {
            int32_t rec[4];
            vsw_record(g->x_max, g->y_max, &s, rec);
            const int64_t row = (int64_t)t * n_traj + i;
            positions[row * 2] = rec[0]; positions[row * 2 + 1] = rec[1];
            if (latents) { latents[row * 4] = rec[0]; latents[row * 4 + 1] = rec[1]; latents[row * 4 + 2] = rec[2]; latents[row * 4 + 3] = rec[3]; }
        }
        vsw_move(g->x_max, g->y_max, &s);
        ++t;
    }
    return 0;
}

// the state from the window: the block that holds the last output consumed (block 0 when none was), pos inside it (1 .. 624, or as found)
VSM_HD void vsw_write_back(uint32_t* state, const uint32_t* raw, int32_t pos, int lane, int nlanes) {
    const int b = pos > 0 ? (pos - 1) / VSM_N : 0;
    for (int i = lane; i < VSM_N; i += nlanes) state[i] = raw[b * VSM_N + i];
    if (lane == 0) state[VSM_N] = (uint32_t)(pos - b * VSM_N);
}

// trajectories [from, to) by the calling lane alone, with the serial reader, from w->pos; leaves w->pos and w->status
VSM_HD void vsw_walk_alone(VswWork* w, const VswGeom* g, int64_t from, int64_t to, int64_t n_traj, const int32_t* start, int32_t* pre,
                           int32_t* positions, int32_t* latents, int32_t* desc, int nd) {
    VswReader r = {w->raw, w->pos, 1};
    for (int64_t i = from; i < to; ++i) {
        const int rc = vsw_trajectory(g, &r, i, n_traj, start, 1, pre, positions, latents, desc, nd);
        if (rc != 0) { w->status = rc; return; }
    }
    w->pos = r.o;
}

// The one-lane form.  state: 625 words, advanced in place on status 0.
VSM_HD int vsw_walk_serial(uint32_t* state, VswWork* w, const VswGeom* g, int64_t n_traj, const int32_t* start, int32_t* pre, int32_t* positions,
                           int32_t* latents, int32_t* desc, int nd) {
    if (state[VSM_N] > VSM_N) return VSM_STATUS_POS;
    for (int i = 0; i < VSM_N; ++i) w->raw[i] = state[i];
    for (int b = 1; b < VSW_BLOCKS; ++b) vsw_regenerate_alone(w->raw + (b - 1) * VSM_N, w->raw + b * VSM_N);
    w->pos = (int32_t)state[VSM_N];
    w->status = VSM_STATUS_OK;
    vsw_walk_alone(w, g, 0, n_traj, n_traj, start, pre, positions, latents, desc, nd);
    if (w->status != VSM_STATUS_OK) return w->status;
    vsw_write_back(state, w->raw, w->pos, 0, 1);
    return VSM_STATUS_OK;
}

// The lanes form.  Every lane calls it with the same arguments; the return value is the same on every lane.
VSM_HD int vsw_walk_lanes(uint32_t* state, VswWork* w, const VswGeom* g, int64_t n_traj, const int32_t* start, int32_t* pre, int32_t* positions,
                          int32_t* latents, int32_t* desc, int nd, int lane, int nlanes) {
    if (state[VSM_N] > VSM_N) return VSM_STATUS_POS;
    for (int i = lane; i < VSM_N; i += nlanes) w->raw[i] = state[i];
    if (lane == 0) { w->pos = (int32_t)state[VSM_N]; w->status = VSM_STATUS_OK; w->made = 0; }
    for (int i = lane; i < 2; i += nlanes) {        // the fixed points of both jump tables
        w->jump[i][VSW_PAST] = VSW_PAST; w->jump[i][VSW_DEAD] = VSW_DEAD;
    }
    VSM_SYNC();
    vsw_fill_window(w->raw, 1, lane, nlanes);       // ends on a barrier
    int64_t done = 0;
    if (g->n_pre < 4) {                             // the walk depends on i, not on the offset alone: one lane
        if (lane == 0) vsw_walk_alone(w, g, 0, n_traj, n_traj, start, pre, positions, latents, desc, nd);
        VSM_SYNC();
        done = n_traj;
    }
    while (done < n_traj && w->status == VSM_STATUS_OK) {
        const int32_t pos = w->pos;
        const int want = n_traj - done < VSW_ROUND ? (int)(n_traj - done) : VSW_ROUND;
        for (int o = pos + lane; o <= VSW_WINDOW; o += nlanes) {                                   // pass 1
            VswReader r = {w->raw, o, 0};
            const int rc = vsw_trajectory(g, &r, 0, n_traj, start, 0, pre, positions, latents, desc, nd);
            w->jump[0][o] = (uint16_t)(rc == 0 ? r.o : rc == VSW_RC_PAST ? VSW_PAST : VSW_DEAD);
        }
        if (lane == 0) w->starts[0] = pos;
        VSM_SYNC();
        int cur = 0;
        for (int step = 1; step <= want; step <<= 1) {                                             // chase: starts[0 .. want]
            const uint16_t* j = w->jump[cur];
            for (int i = lane; i < step && i + step <= want; i += nlanes) w->starts[i + step] = j[w->starts[i]];
            for (int o = pos + lane; o <= VSW_WINDOW; o += nlanes) w->jump[cur ^ 1][o] = j[j[o]];
            VSM_SYNC();
            cur ^= 1;
        }
        for (int i = lane; i <= want; i += nlanes)                                                 // the one i that is the last start inside the window
            if (w->starts[i] <= VSW_WINDOW && (i == want || w->starts[i + 1] > VSW_WINDOW)) {
                w->made = i;
                if (i < want && w->starts[i + 1] == VSW_DEAD) w->status = VSW_STATUS_BOUNCE;
            }
        VSM_SYNC();
        const int made = w->made;
        for (int i = lane; i < made; i += nlanes) {                                                // pass 2
            VswReader r = {w->raw, w->starts[i], 0};
            vsw_trajectory(g, &r, done + i, n_traj, start, 1, pre, positions, latents, desc, nd);
        }
        VSM_SYNC();
        if (w->status != VSM_STATUS_OK) break;
        if (lane == 0) w->pos = w->starts[made];
        done += made;
        VSM_SYNC();
        if (made == 0 && pos <= VSM_N) {            // more outputs than a whole window holds: one lane, which slides the window alone
            if (lane == 0) vsw_walk_alone(w, g, done, done + 1, n_traj, start, pre, positions, latents, desc, nd);
            done += 1;
            VSM_SYNC();
        }
        const int32_t at = w->pos;
        if (done < n_traj && w->status == VSM_STATUS_OK && at > VSM_N) {                           // advance
            vsw_slide(w->raw, (at - 1) / VSM_N, lane, nlanes);
            if (lane == 0) w->pos = at - ((at - 1) / VSM_N) * VSM_N;
            VSM_SYNC();
        }
    }
    const int status = w->status;
    if (status != VSM_STATUS_OK) return status;
    vsw_write_back(state, w->raw, w->pos, lane, nlanes);
    return VSM_STATUS_OK;
}

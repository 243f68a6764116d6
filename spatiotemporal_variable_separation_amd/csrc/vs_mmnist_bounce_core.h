// vs_mmnist_bounce_core.h -- the Moving-MNIST walker of the reference (data/moving_mnist.py:162-255) as plain __host__ __device__ functions:
// a digit's position and speed, the elastic bounce off the frame borders (`_process_collision`) and the record-then-move step, in double
// arithmetic (the reference's Python floats) on the same values in the same order, with no contraction into fused multiply-adds.  It knows
// nothing of the random stream, of lanes or of barriers, and compiles with a host compiler alone (tests/host/mmnist_bounce_host_check.cpp).
//
// Both samplers are this code.  What a collision pass does between computing p and mirroring the speed is its `redraw` argument, a type:
//   * VswKeepSpeed, which is empty -- the deterministic sampler (vsw_walk_deterministic below; csrc/vs_data.hip walks with it);
//   * the stochastic sampler's (csrc/vs_mmnist_walk_core.h), which draws dx, then dy, from the NumPy stream and may fail.
#pragma once
#include <stdint.h>

#ifndef VSW_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define VSW_HD __host__ __device__ inline
#else
#define VSW_HD inline
#endif
#endif

#define VSW_MAX_PASSES 64                           /* collision passes per call after which both samplers give up (s->passes) */

VSW_HD int32_t vsw_abs(int32_t v) { return v < 0 ? -v : v; }

// the walker between two collision passes: position, speed, the collision point of the call in progress, the edges that are hit
struct VswBody {
    double sx, sy, cx, cy;                          // x: rows, y: columns, as in the reference
    int32_t dx, dy, passes;
    bool left, upper, right, bottom;
};

struct VswKeepSpeed {
    VSW_HD int operator()(int32_t*, int32_t*) const { return 0; }
};

// the edges the position lies beyond (moving_mnist.py:196-199, 248-251); with it a new call of the collision function begins or goes on
VSW_HD void vsw_edges(int32_t x_max, int32_t y_max, VswBody* s) {
    const double eps = 1e-8;
    s->left = s->sx < 0.0 - eps; s->upper = s->sy < 0.0 - eps; s->right = s->sx > (double)x_max + eps; s->bottom = s->sy > (double)y_max + eps;
}

VSW_HD VswBody vsw_body(int32_t x_max, int32_t y_max, double sx, double sy, int32_t dx, int32_t dy) {
    VswBody s = {sx, sy, 0.0, 0.0, dx, dy, 0, false, false, false, false};
    vsw_edges(x_max, y_max, &s);
    return s;
}

// ONE pass of the while loop of moving_mnist.py:201-251 (some edge is hit).  left / right exclude each other, and so do upper / bottom, so
// the reference's four intersection tests are two here, in its order, and its two forms of p one division of the selected operands: the
// same operations on the same values.  (cx, cy) live across the passes of one call, as the reference's locals do, and the edge flags
// which the intersection tests cleared stay cleared for the mirroring.  0, or what `redraw` returned (nothing but the speed has changed).
template <class Redraw>
VSW_HD int vsw_pass(int32_t gx_max, int32_t gy_max, VswBody* s, const Redraw& redraw) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double eps = 1e-8, x_min = 0.0, y_min = 0.0, x_max = (double)gx_max, y_max = (double)gy_max;
    ++s->passes;
    if (s->dx == 0) {
        s->cx = s->sx; s->cy = s->upper ? y_min : y_max;
    } else if (s->dy == 0) {
        s->cx = s->left ? x_min : x_max; s->cy = s->sy;
    } else {
        const double a = (double)s->dy / (double)s->dx;
        const double b = s->sy - a * s->sx;
        if (s->left || s->right) {
            const double x_lim = s->left ? x_min : x_max, y = a * x_lim + b;
            const bool hit = (y >= y_min - eps) && (y <= y_max + eps);
            if (s->left) s->left = hit; else s->right = hit;
            if (hit) { s->cx = x_lim; s->cy = y; }
        }
        if (s->upper || s->bottom) {
            const double y_lim = s->upper ? y_min : y_max, x = (y_lim - b) / a;
            const bool hit = (x >= x_min - eps) && (x <= x_max + eps);
            if (s->upper) s->upper = hit; else s->bottom = hit;
            if (hit) { s->cx = x; s->cy = y_lim; }
        }
    }
    const double p = (s->dx != 0 ? s->sx - s->cx : s->sy - s->cy) / (double)(s->dx != 0 ? s->dx : s->dy);
    const int rc = redraw(&s->dx, &s->dy);
    if (rc != 0) return rc;
    if (s->left) s->dx = vsw_abs(s->dx);
    if (s->right) s->dx = -vsw_abs(s->dx);
    if (s->upper) s->dy = vsw_abs(s->dy);
    if (s->bottom) s->dy = -vsw_abs(s->dy);
    s->sx = s->cx + (double)s->dx * p;
    s->sy = s->cy + (double)s->dy * p;
    vsw_edges(gx_max, gy_max, s);
    return 0;
}

// Python's int(round(v)) for a coordinate the collision pass left inside the frame (a NaN, which no stream gives, becomes 0)
VSW_HD int32_t vsw_round(double v, int32_t hi) {
    if (!(v >= -1.0 && v <= (double)hi + 1.0)) return 0;
    return (int32_t)__builtin_rint(v);
}

// moving_mnist.py:166-175 once no edge is hit: the frame's row (rounded position, speed), then the move and the next call of the collision
// function
VSW_HD void vsw_record(int32_t x_max, int32_t y_max, const VswBody* s, int32_t row[4]) {
    row[0] = vsw_round(s->sx, x_max); row[1] = vsw_round(s->sy, y_max); row[2] = s->dx; row[3] = s->dy;
}
VSW_HD void vsw_move(int32_t x_max, int32_t y_max, VswBody* s) {
    s->sy += (double)s->dy;
    s->sx += (double)s->dx;
    s->passes = 0; s->cx = 0.0; s->cy = 0.0;
    vsw_edges(x_max, y_max, s);
}

// The deterministic sampler: frames 0 .. t1 - 1 of the digit that starts at (sx, sy) with speed (dx, dy); the rows of frames t >= t0 go to
// record(t, row).  A call that exhausts its passes (a digit with no room and a speed: the reference never returns) stops bouncing and the
// frame records the position it has, which vsw_round keeps inside [-1, max + 1]; the number of such frames is returned.
template <class Record>
VSW_HD int vsw_walk_deterministic(int32_t x_max, int32_t y_max, int32_t sx, int32_t sy, int32_t dx, int32_t dy, int t0, int t1,
                                   const Record& record) {
    VswBody s = vsw_body(x_max, y_max, sx, sy, dx, dy);
    int gave_up = 0;
    for (int t = 0; t < t1; ++t) {
        while (s.left || s.right || s.upper || s.bottom)
            if (s.passes >= VSW_MAX_PASSES || vsw_pass(x_max, y_max, &s, VswKeepSpeed()) != 0) { ++gave_up; break; }
        if (t >= t0) {
            int32_t row[4];
            vsw_record(x_max, y_max, &s, row);
            record(t, row);
        }
        vsw_move(x_max, y_max, &s);
    }
    return gave_up;
}

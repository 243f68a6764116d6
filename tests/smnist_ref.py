"""A plain restatement of the reference's STOCHASTIC Moving-MNIST sampler (data/moving_mnist.py:131-253 with deterministic=False), driven by
a `rnd(low, high)` callable that stands for the scalar np.random.randint.  TEST INFRASTRUCTURE ONLY: nothing under the package imports it.
tests/make_golden_smnist.py requires it to reproduce the reference's own `_compute_trajectory` value for value before it writes
tests/golden/smnist.npz; the tests then use it, driven by NumPy, as the checker of csrc/vs_mmnist_walk_core.h on every case.

`note(event, value)` (optional) is told what a case has to contain: ('pre', +1 / -1) and ('redraw', +1 / -1) round the prefix draws and
round the two redraws of a pass, ('edges', n) the number of edges hit at the start of a pass, ('passes', n) the passes of one call."""
EPS = 1e-8


def _hit(sx, sy, x_max, y_max):
    return sx < -EPS, sy < -EPS, sx > x_max + EPS, sy > y_max + EPS       # left, upper, right, bottom


def collide(rnd, sx, sy, dx, dy, x_max, y_max, max_speed, note=None):
    left, upper, right, bottom = _hit(sx, sy, x_max, y_max)
    passes = 0
    while left or right or upper or bottom:
        passes += 1
        if note:
            note('edges', left + right + upper + bottom)
        if dx == 0:
            cx, cy = sx, (0 if upper else y_max)
        elif dy == 0:
            cx, cy = (0 if left else x_max), sy
        else:
            a = dy / dx
            b = sy - a * sx
            if left:
                y = a * 0 + b
                left = (y >= -EPS) and (y <= y_max + EPS)
                if left:
                    cx, cy = 0, y
            if right:
                y = a * x_max + b
                right = (y >= -EPS) and (y <= y_max + EPS)
                if right:
                    cx, cy = x_max, y
            if upper:
                x = (0 - b) / a
                upper = (x >= -EPS) and (x <= x_max + EPS)
                if upper:
                    cx, cy = x, 0
            if bottom:
                x = (y_max - b) / a
                bottom = (x >= -EPS) and (x <= x_max + EPS)
                if bottom:
                    cx, cy = x, y_max
        p = (sx - cx) / dx if dx != 0 else (sy - cy) / dy
        if note:
            note('redraw', 1)
        dx = rnd(-max_speed, max_speed + 1)
        dy = rnd(-max_speed, max_speed + 1)
        if note:
            note('redraw', -1)
        if left:
            dx = abs(dx)
        if right:
            dx = -abs(dx)
        if upper:
            dy = abs(dy)
        if bottom:
            dy = -abs(dy)
        sx, sy = cx + dx * p, cy + dy * p
        left, upper, right, bottom = _hit(sx, sy, x_max, y_max)
    if note:
        note('passes', passes)
    return sx, sy, dx, dy


def walk(rnd, start, seq_len, x_max, y_max, max_speed, note=None):
    """[(row, column, row speed, column speed)] * seq_len from the start state (row, column, row speed, column speed)."""
    sx, sy, dx, dy = (int(v) for v in start)
    out = []
    for _ in range(seq_len):
        sx, sy, dx, dy = collide(rnd, sx, sy, dx, dy, x_max, y_max, max_speed, note)
        out.append((int(round(sx)), int(round(sy)), int(dx), int(dy)))
        sy += dy
        sx += dx
    return out


def sample(rnd, n_traj, seq_len, cols, x_max, y_max, max_speed, start=None, note=None):
    """(pre [n_traj][n_pre], trajectories [n_traj][seq_len][4]): per trajectory the prefix draws rnd(low, high) over `cols`, then the walk
    from the last four of them, or from start[i] when there are fewer than four."""
    pre, traj = [], []
    for i in range(n_traj):
        if note:
            note('pre', 1)
        q = [int(rnd(low, high)) for low, high in cols]
        if note:
            note('pre', -1)
        pre.append(q)
        traj.append(walk(rnd, q[-4:] if len(q) >= 4 else start[i], seq_len, x_max, y_max, max_speed, note))
    return pre, traj

"""NumPy restatement of the WaveEq generator (TEST INFRASTRUCTURE ONLY): preprocessing/wave/gen_wave.py:37-92 of the reference integrated with
torchdiffeq's fixed-grid "rk4", which is the 3/8 rule.  `simulate(..., dtype)` runs in the given dtype: float64 is the reference the
GPU tests compare with, float32 is the yardstick for the tolerance (the error an fp32 run of the SAME arithmetic makes).

    y = (w, w'),  y' = (w', c^2 (w_yy + w_xx) + s(t) mask),  s(t) = f0 exp(-20 t),  mask = (col - 32)^2 + (row - 32)^2 < 25
    w_yy[:, i] = -1/12 w[:, i+2] + 4/3 w[:, i+1] - 5/2 w[:, i] + 4/3 w[:, i-1] - 1/12 w[:, i-2]   for i in 2..61, zero in columns 0, 1, 62, 63
    w_xx[j, :] = the same along the first axis                                                     for j in 2..61, zero in rows    0, 1, 62, 63
    k1 = f(t0, y); k2 = f(t0 + h/3, y + h k1 / 3); k3 = f(t0 + 2h/3, y + h (k2 - k1/3)); k4 = f(t1, y + h (k1 - k2 + k3))
    y += (k1 + 3 (k2 + k3) + k4) h / 8

The time grid (fp32 arange), the stage times (formed in fp32) and the source values (fp64 exp, rounded to fp32) are those of the
reference in every dtype: they are the run's inputs; c^2 is rounded to fp32 once likewise.  Only the arithmetic on the fields changes with `dtype`.
"""
import numpy as np

N = 64


def disc():
    cols, rows = np.meshgrid(np.arange(N), np.arange(N))
    return (cols - 32) ** 2 + (rows - 32) ** 2 < 25


def time_grid(T, dt):
    """The reference's grid by the reference's own call (gen_wave.py:134): torch rounds the points of a float32 arange in its own way."""
    import torch
    return torch.arange(0, float(dt) * T, float(dt), dtype=torch.float32)[:T].numpy()


def source_values(f0, t_stage):
    """fp32 times -> f0 * exp(-20 t) in fp64, rounded to fp32 (the Python float meets an fp32 mask in the reference)."""
    return np.float32(float(f0) * np.exp(-20.0 * np.asarray(t_stage, dtype=np.float32).astype(np.float64)))


def accel(w, c2, s, mask):
    yy = np.zeros_like(w)
    xx = np.zeros_like(w)
    a, b, d = w.dtype.type(-1 / 12), w.dtype.type(4 / 3), w.dtype.type(5 / 2)
    e = w.dtype.type(1 / 12)
    yy[:, 2:-2] = a * w[:, 4:] + b * w[:, 3:-1] - d * w[:, 2:-2] + b * w[:, 1:-3] - e * w[:, :-4]
    xx[2:-2, :] = a * w[4:, :] + b * w[3:-1, :] - d * w[2:-2, :] + b * w[1:-3, :] - e * w[:-4, :]
    return s * mask + c2 * (yy + xx)


def simulate(f0, c, T, dt=0.001, init=None, dtype=np.float64):
    """One sequence -> frames [T, 64, 64] in `dtype` (frame i = w after i steps)."""
    ft = np.dtype(dtype).type
    y = np.zeros((2, N, N), dtype) if init is None else np.array(init, dtype=dtype)
    mask = disc().astype(dtype)
    c2 = ft(np.float32(float(c) * float(c)))
    t = time_grid(T, dt)
    third, two_thirds = np.float32(1 / 3), np.float32(2 / 3)
    frames = np.empty((T, N, N), dtype)
    frames[0] = y[0]

    def f(ts, y):
        return np.stack([y[1], accel(y[0], c2, ft(source_values(f0, ts)), mask)])

    for i in range(T - 1):
        h32 = t[i + 1] - t[i]
        h, th = ft(h32), ft(third)
        k1 = f(t[i], y)
        k2 = f(t[i] + h32 * third, y + h * k1 * th)
        k3 = f(t[i] + h32 * two_thirds, y + h * (k2 - k1 * th))
        k4 = f(t[i + 1], y + h * (k1 - k2 + k3))
        y = y + (k1 + ft(3) * (k2 + k3) + k4) * h * ft(0.125)
        frames[i + 1] = y[0]
    return frames


def simulate_many(f0s, cs, T, dt=0.001, init=None, dtype=np.float64):
    return np.stack([simulate(f0, c, T, dt, None if init is None else init[k], dtype) for k, (f0, c) in enumerate(zip(f0s, cs))])

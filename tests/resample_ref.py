"""NumPy restatement of PIL's 8-bit Lanczos resampling (ImagingResample) through a crop box (a plain helper module: tests import it).

Written from the arithmetic itself, independently of `ops.lanczos_coeffs`: per-axis coefficient tables in Python floats (C doubles, math.sin),
22 fractional bits, then the horizontal pass over the rows of the box rounded to uint8 and the vertical pass over that intermediate.
Accumulation is int64 with an assert that every sum fits 32 bits, which is what the kernel has.
"""
import math

import numpy as np

PRECISION_BITS = 22


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3.0)
    return 0.0


def tables(in_size, out_size):
    """(k int32 [out_size, ksize], bounds int32 [out_size, 2] = (xmin, xmax)); entries beyond xmax are 0."""
    scale = (float(in_size) - 0.0) / out_size
    fs = scale if scale > 1.0 else 1.0
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    k = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        ww, w = 0.0, []
        for x in range(xmax):
            v = _lanczos((x + xmin - center + 0.5) / fs)
            w.append(v)
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            k[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5)
        bounds[xx] = (xmin, xmax)
    return k, bounds


def _pass(src, k, bounds):
    """One pass along axis 1 of src uint8 [n, L, ...] -> uint8 [n, out, ...]."""
    out = np.empty((src.shape[0], k.shape[0]) + src.shape[2:], dtype=np.uint8)
    for xx in range(k.shape[0]):
        xmin, xmax = int(bounds[xx, 0]), int(bounds[xx, 1])
        coeff = k[xx, :xmax].astype(np.int64).reshape((1, xmax) + (1,) * (src.ndim - 2))
        ss = (1 << (PRECISION_BITS - 1)) + (src[:, xmin:xmin + xmax].astype(np.int64) * coeff).sum(axis=1)
        assert np.abs(ss).max() < 1 << 31
        out[:, xx] = np.clip(ss >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resample(images, box, size):
    """uint8 [n, H, W, C] -> uint8 [n, size_h, size_w, C]; box = (left, upper, right, lower), size = (w, h) or an int."""
    out_w, out_h = (size, size) if isinstance(size, int) else size
    left, upper, right, lower = box
    crop = np.ascontiguousarray(images[:, upper:lower, left:right])
    kx, bx = tables(right - left, out_w)
    ky, by = tables(lower - upper, out_h)
    tmp = _pass(crop.transpose(0, 2, 1, 3), kx, bx).transpose(0, 2, 1, 3)      # horizontal: over the columns of every row of the box
    return np.ascontiguousarray(_pass(tmp, ky, by))                            # vertical: over the uint8 intermediate


def resample_tensor(images_u8, box, size):
    """The signature of ops.resample_lanczos_u8 on CPU tensors (a stand-in for tests that run without a GPU)."""
    import torch
    return torch.from_numpy(resample(images_u8.cpu().numpy(), tuple(int(v) for v in box), size))

"""Seeded inputs of the resampling cases (tests/test_resample_cpu.py, tests/test_resample_gpu.py, tests/make_golden_resample.py), and the
raw `rendered_chairs` trees the preprocessing tests prepare.  Nothing here imports the reference or PIL.

CASES: name -> (input shape (n, H, W, C), box (left, upper, right, lower), output size (w, h) or an int).  The golden files
tests/golden/resample/<name>.npz hold PIL's outputs for these inputs (key `out`)."""
import os

import numpy as np

import chairs_inputs

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'resample')
SEED = 6262

CASES = {
    'a': ((3, 600, 600, 3), (100, 100, 500, 500), 64),         # the real shape: ksize 39, 76.8 KB of horizontal result per image
    'b': ((2, 50, 70, 3), (3, 5, 60, 45), (16, 16)),           # odd byte offsets, W * C no multiple of 4, another scale per axis
    'c': ((1, 40, 40, 3), (0, 0, 40, 40), 64),                 # upscale: ksize 7, bounds cut at both borders
    'd': ((5, 121, 121, 1), (20, 20, 100, 100), 64),           # scale 1.25, one channel, rows not dword-aligned
    'd4': ((2, 33, 47, 4), (1, 2, 46, 31), (24, 9)),           # four channels
    'e': ((4, 24, 24, 3), (4, 4, 20, 20), 16),                 # scale 1: the output is the cropped input
    'f': ((70, 120, 120, 3), (20, 20, 100, 100), 64),          # more images than one object's 62 views
}


def _edges(rng, H, W, C):
    """Hard 0 / 255 rectangles and stripes: the filter's negative lobes overshoot at both ends, so results clip at 0 and at 255."""
    img = np.zeros((H, W, C), dtype=np.uint8)
    for _ in range(12):
        y0, x0 = rng.randint(0, H), rng.randint(0, W)
        y1, x1 = rng.randint(y0, H) + 1, rng.randint(x0, W) + 1
        img[y0:y1, x0:x1, rng.randint(0, C)] = 255 * rng.randint(0, 2)
    img[:, ::max(W // 9, 2)] = 255
    img[::max(H // 7, 2)] = 0
    return img


def _pattern(H, W, C):
    yy, xx = np.mgrid[0:H, 0:W]
    chans = [(xx * 7 + yy * 3) % 256, ((xx // 5 + yy // 3) % 2) * 255, (xx * yy) % 251, (xx ^ yy) % 256]
    return np.stack(chans[:C], axis=-1).astype(np.uint8)


def case_input(name):
    """uint8 [n, H, W, C]: image 0 random, image 1 hard-edged, image 2 patterned, the others hard-edged again (each its own draw: their
    outputs compress, which keeps the golden files small)."""
    (n, H, W, C), _, _ = CASES[name]
    rng = np.random.RandomState(SEED + sum(ord(ch) for ch in name))
    out = np.empty((n, H, W, C), dtype=np.uint8)
    for i in range(n):
        out[i] = rng.randint(0, 256, size=(H, W, C)) if i == 0 else (_pattern(H, W, C) if i == 2 else _edges(rng, H, W, C))
    return out


def golden(name):
    with np.load(os.path.join(GOLDEN, '%s.npz' % name)) as z:
        return z['out']


# ---- raw rendered_chairs trees ------------------------------------------------------------------------------------------------
RAW_SIZE, RAW_BOX = 120, (20, 20, 100, 100)


def raw_object_names(n_objects):
    return chairs_inputs.object_names()[:n_objects]


def raw_views(k, n_views, size=RAW_SIZE):
    """uint8 [n_views, size, size, 3] of object k: smooth gradients plus a hard-edged square that moves with the view."""
    rng = np.random.RandomState(SEED + 977 * k)
    base = rng.randint(0, 256, size=(3,))
    yy, xx = np.mgrid[0:size, 0:size]
    out = np.empty((n_views, size, size, 3), dtype=np.uint8)
    for v in range(n_views):
        img = np.stack([(xx * 2 + v * 3 + base[0]) % 256, (yy * 2 + k * 17 + base[1]) % 256, ((xx + yy) + v + base[2]) % 256], axis=-1)
        s = 20 + (v * 5 + k * 11) % (size - 60)
        img[s:s + 30, s:s + 30] = (255, 0, 255 * (v % 2))
        out[v] = img.astype(np.uint8)
    return out


def raw_file_names(n_views):
    """Names whose sorted order is not the numeric one and that match no `<digits>.png`: image_000.png ..."""
    return ['image_%03d.png' % v for v in range(n_views)]


def write_raw_tree(data_dir, n_objects, n_views, size=RAW_SIZE):
    """`data_dir/rendered_chairs/<object>/renders/image_<v>.png` (raw renders) + `all_chair_names.mat`; returns data_dir."""
    root = os.path.join(str(data_dir), 'rendered_chairs')
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, 'all_chair_names.mat'), 'wb') as f:
        f.write(b'placeholder: the loaders drop this entry from the listing\n')
    for k, name in enumerate(raw_object_names(n_objects)):
        d = os.path.join(root, name, 'renders')
        os.makedirs(d, exist_ok=True)
        views = raw_views(k, n_views, size)
        for v, fname in enumerate(raw_file_names(n_views)):
            chairs_inputs.write_png(os.path.join(d, fname), views[v], ftype=(k + v) % 3)      # (types 0..2: the vectorised ones, quick to read)
    return str(data_dir)

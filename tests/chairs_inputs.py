"""Inputs of the 3D Chairs fixtures (tests/golden/eval_cli_chairs*), rebuilt from a seed by the fixture generator
(tests/make_golden_eval_cli_chairs.py) and by the tests (tests/test_chairs_cpu.py, tests/test_chairs_gpu.py).  Nothing here imports the
reference.

A tiny `rendered_chairs/` tree in the dataset's layout: N_OBJECTS object directories with `renders/0.png .. 61.png` (64 x 64 8-bit
RGB) and the `all_chair_names.mat` placeholder the reference removes from its listing.  7 objects: the 85 % split leaves 5 for training
and 2 for testing, i.e. 124 test items, a ragged last batch at RUN['batch_size'].  Object k < 5 is written with PNG filter type k on
every row by the stdlib writer below, so that a reader meets all five types; the others are written by PIL (adaptive filters) when it
imports, and by the stdlib writer with the filter type cycling over the rows otherwise.  The PIXELS are the same either way.
"""
import os
import struct
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')

N_OBJECTS, N_VIEWS, SIZE, SEED = 7, 62, 64, 4242
# nt_cond of oracle.golden_configs.CONFIGS['chairs_resnet']; 124 test items in batches of 48, 48, 28
RUN = dict(nt_cond=2, nt_pred=2, batch_size=48, test_seed=1)
PARAMS = dict(architecture='dcgan', data='chairs', nt_cond=2, nt_pred=2, offset=2, skipco=False)
PARAMS_RESNET = dict(architecture='resnet', decoder_architecture='dcgan', data='chairs', nt_cond=2, nt_pred=2, offset=2, skipco=False)


def object_names():
    return ['chair_%s' % tag for tag in ('b7e1', '03fa', 'c210', '9d4e', '5a77', 'e0c3', '18bd')]


def object_views(k):
    """uint8 [62, 64, 64, 3]: a flat background, a soft blob circling the centre once over the 62 views and a bar turning with the view,
    all in colours of object k.  Levels are posterised to multiples of 8 so that the committed arrays compress."""
    rng = np.random.RandomState(SEED + 31 * k)
    bg, blob, bar = rng.randint(32, 224, size=(3, 3)).astype(np.float64)
    radius, width, sharp = rng.uniform(10, 20), rng.uniform(5, 9), rng.uniform(2.5, 5.0)
    yy, xx = np.mgrid[0:SIZE, 0:SIZE].astype(np.float64)
    out = np.empty((N_VIEWS, SIZE, SIZE, 3), dtype=np.uint8)
    for v in range(N_VIEWS):
        a = 2 * np.pi * v / N_VIEWS
        cy, cx = 31.5 + radius * np.sin(a), 31.5 + radius * np.cos(a)
        m_blob = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * width ** 2))
        across = -(yy - 31.5) * np.cos(a + k) + (xx - 31.5) * np.sin(a + k)
        m_bar = 1.0 / (1.0 + np.exp((np.abs(across) - 4.0) * sharp))
        img = bg[None, None] * (1 - m_blob[..., None]) + blob[None, None] * m_blob[..., None]
        img = img * (1 - 0.8 * m_bar[..., None]) + bar[None, None] * 0.8 * m_bar[..., None]
        out[v] = (np.floor(img / 8.0 + 0.5) * 8).clip(0, 255).astype(np.uint8)
    return out


def _filter_row(ftype, cur, prev, bpp=3):
    """PNG filter `ftype` of one row of bytes (int32 in, uint8 out)."""
    left = np.concatenate([np.zeros(bpp, dtype=np.int32), cur[:-bpp]])
    if ftype == 0:
        pred = 0
    elif ftype == 1:
        pred = left
    elif ftype == 2:
        pred = prev
    elif ftype == 3:
        pred = (left + prev) >> 1
    else:
        upleft = np.concatenate([np.zeros(bpp, dtype=np.int32), prev[:-bpp]])
        p = left + prev - upleft
        pa, pb, pc = np.abs(p - left), np.abs(p - prev), np.abs(p - upleft)
        pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, upleft))
    return ((cur - pred) & 255).astype(np.uint8)


def _chunk(kind, body):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body) & 0xffffffff)


def write_png(path, img, ftype=None):
    """8-bit RGB, non-interlaced; every row filtered with `ftype`, or with type (row % 5) when ftype is None."""
    h, w, _ = img.shape
    rows = img.reshape(h, w * 3).astype(np.int32)
    prev = np.zeros(w * 3, dtype=np.int32)
    raw = bytearray()
    for y in range(h):
        f = y % 5 if ftype is None else ftype
        raw.append(f)
        raw += _filter_row(f, rows[y], prev).tobytes()
        prev = rows[y]
    with open(path, 'wb') as fh:
        fh.write(b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0))
                 + _chunk(b'IDAT', zlib.compress(bytes(raw), 6)) + _chunk(b'IEND', b''))


def write_tree(data_dir):
    """`data_dir/rendered_chairs/<object>/renders/<view>.png` + `all_chair_names.mat`; returns data_dir."""
    try:
        from PIL import Image
    except ImportError:
        Image = None
    root = os.path.join(data_dir, 'rendered_chairs')
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, 'all_chair_names.mat'), 'wb') as f:
        f.write(b'placeholder: the loaders drop this entry from the listing\n')
    for k, name in enumerate(object_names()):
        d = os.path.join(root, name, 'renders')
        os.makedirs(d, exist_ok=True)
        views = object_views(k)
        for v in range(N_VIEWS):
            path = os.path.join(d, '%d.png' % v)
            if k < 5:
                write_png(path, views[v], ftype=k)
            elif Image is not None:
                Image.fromarray(views[v], 'RGB').save(path, optimize=True)
            else:
                write_png(path, views[v])
    return data_dir


def split_order(train):
    """[(object name, k)] of a split, in the loaders' order: sorted listing, RandomState(42) shuffle, 85 % cut (chairs.py:34-43)."""
    names = sorted(object_names())
    np.random.RandomState(42).shuffle(names)
    cut = int(len(names) * 0.85)
    pick = names[:cut] if train else names[cut:]
    return [(n, object_names().index(n)) for n in pick]


def split_frames(train):
    """uint8 [n, 62, 64, 64, 3]: what a loader of the split holds."""
    return np.stack([object_views(k) for _, k in split_order(train)])


def expected_item(frames, index, seq_len, chosen_idx=None, chosen_id_st=None):
    """float32 [seq_len, 3, 64, 64] of item `index`: chairs.py:45-64 restated on the decoded split."""
    n = frames.shape[0]
    index, idx = divmod(index, n)
    if chosen_idx is not None:
        idx = chosen_idx
    index, id_st = divmod(index, N_VIEWS)
    if chosen_id_st is not None:
        id_st = chosen_id_st
    assert index == 0
    seq = np.stack([frames[idx, i % N_VIEWS] for i in range(id_st, id_st + seq_len)])
    return (seq / 255).transpose(0, 3, 1, 2).astype(np.float32)


def load_output(directory, name):
    """{key: array} of an output file of a fixture directory: `<name>` itself, or its `<stem>.part<k>.npz` pieces (consecutive items,
    cut by the fixture generator to keep every committed file small) joined along the item axis."""
    path = os.path.join(directory, name)
    if os.path.exists(path):
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    parts, k = [], 0
    while os.path.exists(os.path.join(directory, '%s.part%d.npz' % (name[:-4], k))):
        with np.load(os.path.join(directory, '%s.part%d.npz' % (name[:-4], k))) as z:
            parts.append({key: z[key] for key in z.files})
        k += 1
    if not parts:
        raise FileNotFoundError(path)
    return {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}

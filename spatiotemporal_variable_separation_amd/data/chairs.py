"""3D Warehouse Chairs resident in HBM, batches gathered on the device (reference: var_sep/data/chairs.py:23-67).

The reference opens and decodes `seq_len` PNG files per item on the host, every time the item is drawn: 128 x 15 = 1920 files per
training batch of the README recipe.  The whole train split (~1184 objects x 62 views x 64 x 64 x 3 bytes = 0.9 GB as uint8) is a
small fraction of HBM, so here every view of the split is decoded ONCE, kept on the device as one uint8 [n, 62, 64, 64, 3] tensor (HWC,
as `np.array(Image.open(f))` yields it), and a batch is one gather launch (`vs_chairs_gather`: wrap-around views, / 255, HWC -> CHW)
driven by a [B, 2] table of (object, first view).  Directory handling, the seeded shuffle, the 85 % split and the decomposition of an
item index follow the reference line by line, so that a seeded sampler visits the same sequences in the same order.
"""
import os
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import ops
from .device import DeviceSet, optional_module, require_gpu

MAX_DECODE_WORKERS = 16          # a fixed cap: the machine's CPU count says nothing about the share this process may use

_PNG_MAGIC = b'\x89PNG\r\n\x1a\n'


def _average_row(cur, up, bpp):
    """PNG filter type 3 of one row (bytearray, in place): cur[i] += floor((cur[i - bpp] + up[i]) / 2) (mod 256).  Plain Python
    integers: every byte depends on the one bpp before it, and per-byte NumPy calls would cost far more than the arithmetic."""
    for i in range(len(cur)):
        left = cur[i - bpp] if i >= bpp else 0
        cur[i] = (cur[i] + ((left + up[i]) >> 1)) & 255


def _paeth_row(cur, up, bpp):
    """PNG filter type 4 of one row (bytearray, in place): cur[i] += paeth(cur[i - bpp], up[i], up[i - bpp]) (mod 256)."""
    for i in range(len(cur)):
        a, b, c = (cur[i - bpp], up[i], up[i - bpp]) if i >= bpp else (0, up[i], 0)
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
        cur[i] = (cur[i] + pred) & 255


def read_png_rgb8(path):
    """uint8 [H, W, 3] of a non-interlaced 8-bit RGB PNG, decoded with zlib and NumPy only (all five filter types).  Used when PIL is
    not importable; ValueError for any other kind of file."""
    with open(path, 'rb') as f:
        raw = f.read()
    if raw[:8] != _PNG_MAGIC:
        raise ValueError('%s: not a PNG file' % path)
    pos, idat, header = 8, [], None
    while pos + 8 <= len(raw):
        length, kind = struct.unpack('>I4s', raw[pos:pos + 8])
        body = raw[pos + 8:pos + 8 + length]
        if len(body) != length:
            raise ValueError('%s: truncated PNG chunk' % path)
        if kind == b'IHDR':
            header = struct.unpack('>IIBBBBB', body)
        elif kind == b'IDAT':
            idat.append(body)
        elif kind == b'IEND':
            break
        pos += 12 + length
    if header is None:
        raise ValueError('%s: PNG without a header' % path)
    width, height, depth, colour, _, _, interlace = header
    if depth != 8 or colour != 2 or interlace != 0:
        raise ValueError('%s: an 8-bit non-interlaced RGB PNG is expected (bit depth %d, colour type %d, interlace %d)'
                         % (path, depth, colour, interlace))
    bpp, stride = 3, 3 * width
    try:
        data = np.frombuffer(zlib.decompress(b''.join(idat)), dtype=np.uint8)
    except zlib.error as e:
        raise ValueError('%s: %s' % (path, e))
    if data.size != height * (stride + 1):
        raise ValueError('%s: %d bytes of image data, %d expected' % (path, data.size, height * (stride + 1)))
    data = data.reshape(height, stride + 1)
    out = np.empty((height, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.uint8)
    for y in range(height):
        ftype, cur = int(data[y, 0]), data[y, 1:].copy()
        if ftype == 1:                                   # Sub: running sum over the pixels of the row, modulo 256
            cur = np.cumsum(cur.reshape(width, bpp), axis=0, dtype=np.uint8).reshape(stride)
        elif ftype == 2:                                 # Up
            cur += prev
        elif ftype in (3, 4):                            # Average / Paeth: sequential along the row
            row = bytearray(cur.tobytes())
            (_average_row if ftype == 3 else _paeth_row)(row, prev.tobytes(), bpp)
            cur = np.frombuffer(bytes(row), dtype=np.uint8)
        elif ftype != 0:
            raise ValueError('%s: unknown PNG filter type %d' % (path, ftype))
        out[y] = cur
        prev = cur
    return out.reshape(height, width, 3)


def _pil_image():
    return optional_module('PIL.Image')


def read_frame(path, size=64, image_module=None):
    """uint8 [size, size, 3] of one rendered view: `np.array(Image.open(path))` (chairs.py:58) when PIL imports, the built-in reader
    otherwise.  A file that is missing or is not a size x size 8-bit RGB image raises ValueError naming it."""
    if not os.path.isfile(path):
        raise ValueError('%s: missing' % path)
    if image_module is not None:
        try:
            with image_module.open(path) as im:
                arr = np.array(im)
        except Exception as e:                           # PIL raises its own error types for files it cannot read
            raise ValueError('%s: %s' % (path, e))
    else:
        arr = read_png_rgb8(path)
    if arr.dtype != np.uint8 or arr.shape != (size, size, 3):
        raise ValueError('%s: a %d x %d 8-bit RGB image is expected (got %s %s)' % (path, size, size, arr.dtype, arr.shape))
    return arr


class Chairs(DeviceSet):
    """`Chairs(train, data_root, nt_cond, seq_len, image_size)` (chairs.py:23-67) with the split's views on `device`."""

    max_length = 62

    def __init__(self, train, data_root, nt_cond, seq_len=15, image_size=64, device=None):
        self.train, self.nt_cond = train, nt_cond
        if seq_len > self.max_length:                    # chairs.py:29
            raise ValueError('seq_len %d exceeds the %d views of an object' % (seq_len, self.max_length))
        if seq_len < 1:
            raise ValueError('seq_len must be at least 1')
        if image_size != 64:                             # chairs.py:31
            raise ValueError('the rendered chairs are 64 x 64 images')
        self.seq_len, self.image_size = seq_len, image_size
        self.device = device = require_gpu('Chairs', device)
        self.data_root = os.path.join(data_root, 'rendered_chairs')
        self.sequences = sorted(os.listdir(self.data_root))
        self.sequences.remove('all_chair_names.mat')
        rng = np.random.RandomState(42)
        rng.shuffle(self.sequences)
        if self.train:
            self.start_idx, self.stop_idx = 0, int(len(self.sequences) * 0.85)
        else:
            self.start_idx, self.stop_idx = int(len(self.sequences) * 0.85), len(self.sequences)
        if self.stop_idx <= self.start_idx:
            raise ValueError('no objects in the %s split of %s' % ('train' if train else 'test', self.data_root))
        self.frames = torch.from_numpy(self._decode_split()).to(device)

    @property
    def n_objects(self):
        return self.stop_idx - self.start_idx

    def _decode_split(self):
        """uint8 [n, 62, 64, 64, 3]: `renders/0.png .. 61.png` of the split's own objects, in the split's order."""
        image_module = _pil_image()
        size = self.image_size
        names = [os.path.join(self.data_root, obj, 'renders', '%d.png' % v)
                 for obj in self.sequences[self.start_idx:self.stop_idx] for v in range(self.max_length)]
        out = np.empty((len(names), size, size, 3), dtype=np.uint8)

        def decode(i):
            out[i] = read_frame(names[i], size, image_module)

        with ThreadPoolExecutor(max_workers=min(MAX_DECODE_WORKERS, len(names))) as pool:
            for _ in pool.map(decode, range(len(names)), chunksize=1):
                pass
        return out.reshape(self.n_objects, self.max_length, size, size, 3)

    def __len__(self):
        return self.max_length * self.n_objects

    def descriptors(self, indices, chosen_idx=None, chosen_id_st=None):
        """int32 [B, 2] = (object within the split, first view) of the items: the decomposition of chairs.py:46-54.  `chosen_idx` /
        `chosen_id_st` override the object / first view per item, as `get_sequence`'s arguments do."""
        index = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        index, idx = np.divmod(index, self.n_objects)
        if chosen_idx is not None:
            idx = np.broadcast_to(np.asarray(chosen_idx, dtype=np.int64), idx.shape)
        index, id_st = np.divmod(index, self.max_length)
        if chosen_id_st is not None:
            id_st = np.broadcast_to(np.asarray(chosen_id_st, dtype=np.int64), id_st.shape)
        if np.any(index != 0):                           # chairs.py:54 asserts
            raise IndexError('an item index is outside the %d items of the set' % len(self))
        if np.any((idx < 0) | (idx >= self.n_objects)) or np.any((id_st < 0) | (id_st >= self.max_length)):
            raise IndexError('an object or first view is outside the %d objects x %d views of the set' % (self.n_objects, self.max_length))
        return np.stack([idx, id_st], axis=1).astype(np.int32)

    def gather(self, desc, out_dtype=torch.float32):
        """[rows, seq_len, 3, 64, 64] of a host descriptor table, one launch; the table has been range-checked on the host, so the
        launch's error word is not read back (no host sync per batch)."""
        desc = torch.from_numpy(np.ascontiguousarray(desc, dtype=np.int32)).to(self.device, non_blocking=True)
        return ops.chairs_gather(self.frames, desc, self.seq_len, out_dtype, validate=False)

    def batch(self, item_idx, out_dtype=torch.float32):
        """item_idx: list of ints (or an integer tensor) [B] -> (cond [B, nt_cond, 3, 64, 64], target [B, seq_len - nt_cond, ...])."""
        if isinstance(item_idx, torch.Tensor):
            item_idx = item_idx.cpu().tolist()
        x = self.gather(self.descriptors(item_idx), out_dtype)
        return x[:, :self.nt_cond], x[:, self.nt_cond:]

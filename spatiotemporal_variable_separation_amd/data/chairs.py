"""3D Warehouse Chairs resident in HBM, batches gathered on the device (reference: var_sep/data/chairs.py:23-67).

The reference opens and decodes `seq_len` PNG files per item on the host, every time the item is drawn: 128 x 15 = 1920 files per
training batch of the README recipe.  The whole train split (~1184 objects x 62 views x 64 x 64 x 3 bytes = 0.9 GB as uint8) is a
small fraction of HBM, so here every view of the split is decoded ONCE, kept on the device as one uint8 [n, 62, 64, 64, 3] tensor (HWC,
as `np.array(Image.open(f))` yields it), and a batch is one gather launch (`vs_chairs_gather`: wrap-around views, / 255, HWC -> CHW)
driven by a [B, 2] table of (object, first view).  Directory handling, the seeded shuffle, the 85 % split and the decomposition of an
item index follow the reference line by line, so that a seeded sampler visits the same sequences in the same order.

The 64 x 64 views are the output of the reference's preprocessing/chairs/gen_chairs.py over the original 600 x 600 renders (crop, Lanczos
resize).  That step runs on the device here (ops.resample_lanczos_u8, PIL's arithmetic bit for bit): preprocessing/chairs/gen_chairs.py
writes the files, `Chairs.from_raw` fills `frames` from the raw renders without writing any.

The raw renders themselves can be decoded on the device too (ops.png_decode_rgb8: inflate + row filters, csrc/vs_png.hip): only the
compressed bytes are uploaded, and the bytes are the host route's.  `decode='host' | 'device'` of `prepare_renders`, `gen_chairs.generate`
and `Chairs.from_raw` selects the decoder; None reads the environment variable VARSEP_CHAIRS_DECODE (`host` or `device`), and when that is
unset the device decodes where PIL does not import and the target is a GPU, the host otherwise (`chairs_decoder`).
"""
import os
import re
import struct
import time
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


class PngNotCovered(ValueError):
    """A file that may well be a valid image, but not one the device decoder covers (8-bit non-interlaced RGB PNG)."""


def png_chunks(raw, path):
    """(IHDR fields (width, height, depth, colour, compression, filter, interlace), [IDAT bodies]) of the bytes of a PNG file: signature,
    IHDR, the IDAT chunks up to IEND.  ValueError naming `path` for a file without the signature (PngNotCovered), a truncated chunk or a
    missing header."""
    if raw[:8] != _PNG_MAGIC:
        raise PngNotCovered('%s: not a PNG file' % path)
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
    return header, idat


def read_png_rgb8(path):
    """uint8 [H, W, 3] of a non-interlaced 8-bit RGB PNG, decoded with zlib and NumPy only (all five filter types).  Used when PIL is
    not importable; ValueError for any other kind of file."""
    with open(path, 'rb') as f:
        raw = f.read()
    header, idat = png_chunks(raw, path)
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
    otherwise.  A file that is missing or is not a size x size 8-bit RGB image raises ValueError naming it.  size=None accepts an 8-bit
    RGB image of any size (the raw renders, which the caller checks against its crop box)."""
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
    if size is None:
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
            raise ValueError('%s: an 8-bit RGB image is expected (got %s %s)' % (path, arr.dtype, arr.shape))
    elif arr.dtype != np.uint8 or arr.shape != (size, size, 3):
        raise ValueError('%s: a %d x %d 8-bit RGB image is expected (got %s %s)' % (path, size, size, arr.dtype, arr.shape))
    return arr


def _png_chunk(kind, body):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body) & 0xffffffff)


def write_png_rgb8(path, img):
    """Writes uint8 [H, W, 3] as a non-interlaced 8-bit RGB PNG with zlib and NumPy only: every row with filter type 2 (Up), one
    vectorised subtraction.  Used when PIL is not importable; `read_png_rgb8` and PIL read back the same pixels."""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError('%s: uint8 [H, W, 3] expected (got %s %s)' % (path, img.dtype, img.shape))
    h, w, _ = img.shape
    rows = img.reshape(h, w * 3)
    raw = np.empty((h, w * 3 + 1), dtype=np.uint8)
    raw[:, 0] = 2
    raw[0, 1:] = rows[0]
    raw[1:, 1:] = rows[1:] - rows[:-1]                   # modulo 256
    with open(path, 'wb') as f:
        f.write(_PNG_MAGIC + _png_chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0))
                + _png_chunk(b'IDAT', zlib.compress(raw.tobytes(), 6)) + _png_chunk(b'IEND', b''))


# ---- the raw renders (600 x 600 in the original set) and their preparation on the device ------------------------------------------
RAW_BOX = (100, 100, 500, 500)                           # gen_chairs.py:31 of the reference
OBJECTS_PER_BATCH = 8                                    # 8 x 62 raw renders of 600 x 600 = 536 MB on the host and in HBM, 1984 workgroups per launch
_PREPARED = re.compile(r'^\d+\.png$')


def list_objects(data_root):
    """(rendered_chairs directory, its sorted entries without `all_chair_names.mat`): the listing of chairs.py:34-35."""
    root = os.path.join(data_root, 'rendered_chairs')
    objects = sorted(os.listdir(root))
    objects.remove('all_chair_names.mat')
    return root, objects


def raw_render_names(renders_dir):
    """`sorted(os.listdir(renders_dir))` (gen_chairs.py:29) without the names `<digits>.png`: those are the files the preparation itself
    writes, which the reference would feed back in on a second run."""
    return [f for f in sorted(os.listdir(renders_dir)) if not _PREPARED.match(f)]


def decode_renders(paths, box, image_module=None):
    """uint8 [n, H, W, 3] of raw renders, decoded on at most MAX_DECODE_WORKERS threads.  ValueError naming the file for one that is no
    8-bit RGB image, does not contain `box` = (left, upper, right, lower), or differs in size from the first of the batch."""
    left, upper, right, lower = box
    if not (0 <= left < right and 0 <= upper < lower):
        raise ValueError('the crop box %s is empty' % (tuple(box),))
    first = read_frame(paths[0], None, image_module)
    out = np.empty((len(paths),) + first.shape, dtype=np.uint8)

    def decode(i):
        arr = first if i == 0 else read_frame(paths[i], None, image_module)
        if right > arr.shape[1] or lower > arr.shape[0]:
            raise ValueError('%s: the crop box %s is not inside the %d x %d image' % (paths[i], tuple(box), arr.shape[1], arr.shape[0]))
        if arr.shape != first.shape:
            raise ValueError('%s: a %d x %d image among %d x %d ones (a batch is one tensor)'
                             % (paths[i], arr.shape[1], arr.shape[0], first.shape[1], first.shape[0]))
        out[i] = arr

    with ThreadPoolExecutor(max_workers=min(MAX_DECODE_WORKERS, len(paths))) as pool:
        for _ in pool.map(decode, range(len(paths)), chunksize=1):
            pass
    return out


DECODE_ENV = 'VARSEP_CHAIRS_DECODE'


def chairs_decoder(decode=None, device=None):
    """'host' or 'device': who decodes the raw renders.  The keyword wins; None reads the environment variable VARSEP_CHAIRS_DECODE; when that
    is unset (or empty) the device decodes where PIL does not import and `device` is a GPU, and the host does otherwise."""
    source = 'decode'
    if decode is None:
        decode, source = os.environ.get(DECODE_ENV) or None, DECODE_ENV
    if decode is None:
        on_gpu = device is not None and torch.device(device).type == 'cuda'
        return 'device' if _pil_image() is None and on_gpu else 'host'
    if decode not in ('host', 'device'):
        raise ValueError("%s must be 'host' or 'device' (got %r)" % (source, decode))
    return decode


ENCODE_ENV = 'VARSEP_CHAIRS_ENCODE'


def chairs_encoder(encode=None):
    """'host' or 'device': who encodes the prepared views of gen_chairs.  The keyword wins; None reads the environment variable
    VARSEP_CHAIRS_ENCODE; unset (or empty) means 'host' on every machine: the device route is opt-in."""
    source = 'encode'
    if encode is None:
        encode, source = os.environ.get(ENCODE_ENV) or 'host', ENCODE_ENV
    if encode not in ('host', 'device'):
        raise ValueError("%s must be 'host' or 'device' (got %r)" % (source, encode))
    return encode


def write_files(paths, files, sizes):
    """files uint8 [n, stride] and sizes int64 [n] (host arrays): files[i, :sizes[i]] into paths[i], on at most MAX_DECODE_WORKERS threads."""
    def write(i):
        with open(paths[i], 'wb') as f:
            f.write(memoryview(files[i, :sizes[i]]))

    with ThreadPoolExecutor(max_workers=min(MAX_DECODE_WORKERS, len(paths))) as pool:
        for _ in pool.map(write, range(len(paths)), chunksize=1):
            pass


def read_files(paths):
    """The bytes of every file, read on at most MAX_DECODE_WORKERS threads; ValueError naming a file that is missing."""
    def read(path):
        if not os.path.isfile(path):
            raise ValueError('%s: missing' % path)
        with open(path, 'rb') as f:
            return f.read()

    with ThreadPoolExecutor(max_workers=min(MAX_DECODE_WORKERS, len(paths))) as pool:
        return list(pool.map(read, paths, chunksize=1))


def _prepare_on_device(paths, box, image_size, device, timings):
    """The device route of `prepare_renders`, or None when a file of the batch is not one the kernels cover."""
    left, upper, right, lower = box
    if not (0 <= left < right and 0 <= upper < lower):
        raise ValueError('the crop box %s is empty' % (tuple(box),))
    t0 = time.perf_counter()
    try:
        width, height, packed, offsets = ops.png_pack(read_files(paths), paths)
    except PngNotCovered:
        return None
    if right > width or lower > height:
        raise ValueError('%s: the crop box %s is not inside the %d x %d image' % (paths[0], tuple(box), width, height))
    t1 = time.perf_counter()
    packed_d, offsets_d = torch.from_numpy(packed).to(device), torch.from_numpy(offsets).to(device)
    if timings is not None:
        torch.cuda.synchronize(device)
    t2 = time.perf_counter()
    pixels, status = ops.png_decode_packed(packed_d, offsets_d, height, width, 3)
    out = ops.resample_lanczos_u8(pixels, box, image_size)
    err = ops.png_status_error(status, paths)             # (reads the statuses back: the three launches are complete)
    if err is not None:
        raise err
    if timings is not None:
        for key, dt in (('decode', t1 - t0), ('upload', t2 - t1), ('kernel', time.perf_counter() - t2)):
            timings[key] = timings.get(key, 0.0) + dt
    return out


def prepare_renders(paths, box, image_size, device, image_module=None, timings=None, decode=None):
    """uint8 [n, image_size, image_size, 3] on `device`: the raw renders cropped to `box` and resized with PIL's Lanczos filter.
    decode (see `chairs_decoder`) = 'host': decode on the host, ONE upload of the pixels, ONE launch (ops.resample_lanczos_u8).
    'device': the files are read and their compressed streams packed on the host, the COMPRESSED bytes are uploaded, and three launches
    (inflate, row filters, resample) do the rest -- the same bytes; a file whose decoding fails raises ValueError naming it and the reason.
    If a file of the batch is an image the kernels do not cover (an interlaced PNG, say), the whole batch takes the host route.
    timings: optional dict; seconds are added to 'decode' (host: decoding; device: reading and packing), 'upload' (host: the pixels;
    device: the compressed bytes) and 'kernel' (all launches), and the device is synchronised after each stage."""
    if chairs_decoder(decode, device) == 'device':
        out = _prepare_on_device(paths, tuple(int(v) for v in box), image_size, device, timings)
        if out is not None:
            return out
    t0 = time.perf_counter()
    raw = decode_renders(paths, box, image_module)
    t1 = time.perf_counter()
    raw_d = torch.from_numpy(raw).to(device)
    if timings is not None:
        torch.cuda.synchronize(device)
    t2 = time.perf_counter()
    out = ops.resample_lanczos_u8(raw_d, box, image_size)
    if timings is not None:
        torch.cuda.synchronize(device)
        for key, dt in (('decode', t1 - t0), ('upload', t2 - t1), ('kernel', time.perf_counter() - t2)):
            timings[key] = timings.get(key, 0.0) + dt
    return out


class Chairs(DeviceSet):
    """`Chairs(train, data_root, nt_cond, seq_len, image_size)` (chairs.py:23-67) with the split's views on `device`."""

    max_length = 62

    @classmethod
    def from_raw(cls, train, data_root, nt_cond, seq_len=15, image_size=64, box=RAW_BOX, device=None, decode=None):
        """The same set built straight from the RAW renders (`renders/<any name>.png`, 600 x 600 in the original set; exactly 62 per
        object), with no files written: every view is decoded, cropped to `box` and resized on the device (ops.resample_lanczos_u8) as
        preprocessing/chairs/gen_chairs.py would prepare it.  Same listing, shuffle and split: `frames` holds the bytes of
        `Chairs(...)` on a tree that `gen_chairs.generate` prepared.  The constructor itself runs, with its own signature (a subclass
        such as the content-swap set of test/chairs/test_disentanglement.py needs no change); it finds the box on the instance, and
        `decode` ('host', 'device' or None: see `chairs_decoder`) likewise."""
        self = cls.__new__(cls)
        self.raw_box = tuple(int(v) for v in box)
        self.raw_decode = decode
        self.__init__(train, data_root, nt_cond, seq_len=seq_len, image_size=image_size, device=device)
        return self

    raw_box = None                                       # set per instance by `from_raw`, before the constructor runs
    raw_decode = None                                    # likewise: who decodes the raw renders

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
        self.data_root, self.sequences = list_objects(data_root)
        rng = np.random.RandomState(42)
        rng.shuffle(self.sequences)
        if self.train:
            self.start_idx, self.stop_idx = 0, int(len(self.sequences) * 0.85)
        else:
            self.start_idx, self.stop_idx = int(len(self.sequences) * 0.85), len(self.sequences)
        if self.stop_idx <= self.start_idx:
            raise ValueError('no objects in the %s split of %s' % ('train' if train else 'test', self.data_root))
        self.frames = torch.from_numpy(self._decode_split()).to(device) if self.raw_box is None else self._prepare_split(self.raw_box)

    @property
    def n_objects(self):
        return self.stop_idx - self.start_idx

    def _prepare_split(self, box):
        """uint8 [n, 62, 64, 64, 3] on the device from the raw renders of the split's own objects, OBJECTS_PER_BATCH objects per launch."""
        image_module = _pil_image()
        size = self.image_size
        objects = self.sequences[self.start_idx:self.stop_idx]
        frames = torch.empty((len(objects), self.max_length, size, size, 3), dtype=torch.uint8, device=self.device)
        for start in range(0, len(objects), OBJECTS_PER_BATCH):
            paths = []
            for obj in objects[start:start + OBJECTS_PER_BATCH]:
                renders = os.path.join(self.data_root, obj, 'renders')
                names = raw_render_names(renders)
                if len(names) != self.max_length:
                    raise ValueError('%s: %d raw renders, exactly %d are expected' % (os.path.join(self.data_root, obj), len(names), self.max_length))
                paths += [os.path.join(renders, f) for f in names]
            out = prepare_renders(paths, box, size, self.device, image_module, decode=self.raw_decode)
            frames[start:start + len(paths) // self.max_length] = out.view(-1, self.max_length, size, size, 3)
        return frames

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

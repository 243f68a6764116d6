"""Inputs and checks of the PNG encoding tests (tests/test_png_encode_cpu.py, tests/test_png_encode_gpu.py): the cases, the case file of
tests/host/png_encode_host_check.cpp and its output, and the checks every encoded file must pass.  The references are tests/png_inputs.py's
`filter_rows` / `adaptive_ftypes` for the rows and `zlib` of the standard library for the streams and both checksums."""
import struct
import subprocess
import zlib

import numpy as np

import host_build
import png_inputs as P
from spatiotemporal_variable_separation_amd.data import chairs as C

ADAPTIVE = 5
FIXED_BYTES = 65                   # 57 + 8
SLOT_EXTRA = 10
DEFAULT_CHUNK = 32768
COLOUR = {1: 0, 2: 4, 3: 2, 4: 6}
MATCH = {'runs': 0, 'window': 1}

# (H, W, C): what the shape reaches
FILTER_SHAPES = ((1, 1, 3), (2, 1, 1), (3, 5, 3), (5, 22, 3), (7, 21, 2), (4, 64, 4), P.PNG_SIZE + (3,))
# (n, (H, W, C), chunk_bytes or None for the default): what png_encode_u8 is called for
ENCODE_CASES = ((1, (1, 1, 3), None), (5, (1, 1, 3), None), (1, (37, 53, 3), None), (5, (37, 53, 3), None), (1, (64, 64, 3), None),
                (5, (64, 64, 3), None), (5, (37, 53, 3), 1024), (1, (130, 130, 3), None), (5, (37, 53, 1), None), (5, (37, 53, 2), None),
                (5, (37, 53, 4), None))


def images(n, shape, seed=0):
    """uint8 [n, H, W, C]: n DIFFERENT images (tests/png_inputs.py's `sample_image`, each its own seed)."""
    h, w, c = shape
    return np.stack([P.sample_image(h, w, c, seed=seed + 17 * i + 1) for i in range(n)])


def special_images(shape=(6, 22, 3)):
    """{name: uint8 [3, H, W, C]}: a constant and an all-zero image (ties between the types) and 0x80 / 0x7F stripes (the signed reading:
    as unsigned bytes 0x7F would cost less than 0x80, as signed ones it costs 127 against 128)."""
    h, w, c = shape
    const = np.full((3, h, w, c), 0x5A, dtype=np.uint8)
    const[1] = 0xFF
    const[2] = 0x01
    stripes = np.empty((3, h, w, c), dtype=np.uint8)
    stripes[0, ::2], stripes[0, 1::2] = 0x80, 0x7F
    stripes[1, :, ::2], stripes[1, :, 1::2] = 0x80, 0x7F
    stripes[2] = np.where((np.arange(h * w * c).reshape(h, w, c) % 3) == 0, 0x80, 0x7F)
    return {'constant': const, 'zero': np.zeros((3, h, w, c), dtype=np.uint8), 'stripes': stripes}


def filtered(imgs, mode):
    """bytes [n][S]: the reference rows of every image for `mode` (0..4, or ADAPTIVE)."""
    return [P.filter_rows(img, P.adaptive_ftypes(img) if mode == ADAPTIVE else [mode] * img.shape[0]) for img in imgs]


def compile_host_check(tmp_path):
    """tests/host/png_encode_host_check.cpp.  (exe, sanitized)."""
    return host_build.compile_host_check(tmp_path, 'png_encode_host_check', start_args=[str(tmp_path / 'empty.out')])


def run_host_check(exe, cases, tmp_path, tag='encode'):
    """The host build on `cases` = [(uint8 [n, H, W, C], mode, chunk_bytes, match name)] -> ([(raw rows [n] bytes, files [n] bytes)], stdout)."""
    path, out = str(tmp_path / (tag + '_cases.bin')), str(tmp_path / (tag + '_out.bin'))
    with open(path, 'wb') as f:
        f.write(struct.pack('<q', len(cases)))
        for imgs, mode, chunk, match in cases:
            n, h, w, c = imgs.shape
            f.write(struct.pack('<7q', n, h, w, c, mode, chunk, MATCH[match]) + np.ascontiguousarray(imgs).tobytes())
    r = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    blob = open(out, 'rb').read()
    assert struct.unpack_from('<q', blob, 0)[0] == len(cases)
    at, records = 8, []
    for _ in cases:
        n, S = struct.unpack_from('<qq', blob, at)
        at += 16
        raws = [blob[at + i * S:at + (i + 1) * S] for i in range(n)]
        at += n * S
        files = []
        for _ in range(n):
            size = struct.unpack_from('<q', blob, at)[0]
            files.append(blob[at + 8:at + 8 + size])
            at += 8 + size
        records.append((raws, files))
    assert at == len(blob)
    return records, r.stdout


def check_file(blob, img, raw, name='file'):
    """Everything one encoded file must satisfy: the chunk sequence with the CRCs of `zlib.crc32`, the header of img's shape, the zlib
    framing with the trailer of `zlib.adler32`, a stream that inflates to `raw` (the reference rows), and pixels that come back."""
    h, w, c = img.shape
    assert blob[:8] == P.MAGIC, name
    at, kinds, idat = 8, [], None
    while at < len(blob):
        length, kind = struct.unpack_from('>I4s', blob, at)
        body = blob[at + 8:at + 8 + length]
        assert len(body) == length, (name, kind)
        assert struct.unpack_from('>I', blob, at + 8 + length)[0] == zlib.crc32(kind + body) & 0xffffffff, (name, kind)
        kinds.append(kind)
        if kind == b'IDAT':
            idat = body
        at += 12 + length
    assert at == len(blob) and kinds == [b'IHDR', b'IDAT', b'IEND'], (name, kinds)
    header, bodies = C.png_chunks(blob, name)
    assert header == (w, h, 8, COLOUR[c], 0, 0, 0) and bodies == [idat], (name, header)
    assert idat[:2] == b'\x78\x9c' and idat[-6:-4] == b'\x03\x00', name
    assert struct.unpack('>I', idat[-4:])[0] == zlib.adler32(raw) & 0xffffffff, name
    assert zlib.decompress(idat) == raw, name
    return idat


def read_back(path_or_blob, tmp_path=None):
    """The pixels `read_png_rgb8` returns for an RGB file given as a path or as bytes."""
    if isinstance(path_or_blob, (bytes, bytearray)):
        path = str(tmp_path / 'read_back.png')
        with open(path, 'wb') as f:
            f.write(path_or_blob)
        path_or_blob = path
    return C.read_png_rgb8(path_or_blob)

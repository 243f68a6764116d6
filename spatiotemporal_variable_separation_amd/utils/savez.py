"""`np.savez_compressed` for mappings that mix host arrays and device tensors, and the rule that says who compresses: the one writer of the
Moving-MNIST test-set file (preprocessing/mnist/make_test_set.py) and of the evaluation scripts' result files (test/mnist/test.py,
test/utils.run_content_swap).

Who compresses: the environment variable VARSEP_NPZ_COMPRESS=host|device (`compress=` in code; the keyword wins, then the variable, then
the default `host`).  `host` downloads every tensor and calls np.savez_compressed: the call and the bytes of the time before the device
encoder existed.  `device` compresses every device tensor in HBM (ops.deflate_raw_slabs: csrc/vs_deflate.hip, run matching + dynamic
Huffman codes per 32 KiB chunk; ops.crc32), downloads only the compressed bytes, lets host zlib compress the host arrays (the small float
files), and writes all members into one zip container (utils/npz.py, which stays host-only); np.load reads either file to the same arrays.

Which matcher the device encoder uses: VARSEP_NPZ_MATCH=runs|window (`match=` in code; keyword, then variable, then the default `runs`).
`runs` knows literals and byte runs: the bytes of the time before the window search existed.  `window` also matches up to 32768 bytes
back (ops.deflate_raw_slabs(match='window'): vs_deflate_chunks_window), which is what a video-major result file needs -- the previous frame
of the same video lies 4096 bytes back -- and costs more time per byte.  The rule matters for `device` only; a bad value is refused always.
"""
import os
import time
import zlib

import numpy as np
import torch

from .. import ops
from . import npz

COMPRESS_ENV = 'VARSEP_NPZ_COMPRESS'
MATCH_ENV = 'VARSEP_NPZ_MATCH'


def npz_compressor(compress=None):
    """'host' or 'device': who compresses an .npz file.  The keyword wins; None reads the environment variable VARSEP_NPZ_COMPRESS; when
    that is unset or empty the host does (np.savez_compressed, the behaviour before the device encoder existed).  Any other value raises,
    naming the two."""
    source = 'compress'
    if compress is None:
        compress, source = os.environ.get('VARSEP_NPZ_COMPRESS', '') or 'host', COMPRESS_ENV
    if compress not in ('host', 'device'):
        raise ValueError("%s=%r: 'host' or 'device' expected" % (source, compress))
    return compress


def npz_matcher(match=None):
    """'runs' or 'window': the matcher of the device encoder.  The keyword wins; None reads the environment variable VARSEP_NPZ_MATCH; when
    that is unset or empty it is 'runs' (the bytes before the window search existed).  Any other value raises, naming the two."""
    source = 'match'
    if match is None:
        match, source = os.environ.get('VARSEP_NPZ_MATCH', '') or 'runs', MATCH_ENV
    if match not in ('runs', 'window'):
        raise ValueError("%s=%r: 'runs' or 'window' expected" % (source, match))
    return match


def device_member(name, t, slab_bytes=None, match='runs'):
    """The npz.Member of a device tensor (made contiguous): its pieces are compressed on the device one slab of `slab_bytes` of input at
    a time as the writer consumes them, and only the compressed bytes are downloaded; its CRC is computed on the device.  match: 'runs'
    (the call of the time before the window search) or 'window'; the member's .npy header, which host zlib writes, is no history."""
    t = t.contiguous()
    header = npz.npy_header(tuple(t.shape), npz.numpy_dtype(t.dtype))
    slabs = ops.deflate_raw_slabs(t, slab_bytes=slab_bytes) if match == 'runs' else ops.deflate_raw_slabs(t, slab_bytes=slab_bytes, match=match)
    return npz.Member(name + '.npy', header, (piece.cpu().numpy() for piece, _ in slabs), ops.crc32(t, init=zlib.crc32(header)),
                      t.numel() * t.element_size())


def savez_compressed(path, arrays, compress=None, timings=None, slab_bytes=None, match=None):
    """Writes `arrays` (an ordered mapping of name -> NumPy array or tensor) to the .npz file `path`, members in the mapping's order.
    compress: 'host' (tensors are downloaded; np.savez_compressed(path, **arrays)), 'device' (every device tensor is a `device_member`,
    every host array and CPU tensor an npz.host_member; one npz.write_npz) or None (`npz_compressor`).  timings: optional dict that
    receives the seconds of 'download' + 'write' (host) or of 'write' (device: compression, download of the compressed bytes and file
    together).  slab_bytes: input bytes per compression pass of the device route (default ops.DEFLATE_SLAB_BYTES).  match: 'runs', 'window'
    or None (`npz_matcher`), resolved once, before anything is compressed; it only matters for 'device'."""
    compress = npz_compressor(compress)
    match = npz_matcher(match)
    t0 = time.perf_counter()
    if compress == 'host':
        host = {k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in arrays.items()}
        t1 = time.perf_counter()
        np.savez_compressed(path, **host)
        if timings is not None:
            timings.update(download=t1 - t0, write=time.perf_counter() - t1)
        return
    members = []
    for name, v in arrays.items():
        if isinstance(v, torch.Tensor) and v.is_cuda:
            members.append(device_member(name, v, slab_bytes) if match == 'runs' else device_member(name, v, slab_bytes, match))
        else:
            members.append(npz.host_member(name, v.numpy() if isinstance(v, torch.Tensor) else v))
    if isinstance(path, str) and not path.endswith('.npz'):               # as np.savez does
        path = path + '.npz'
    npz.write_npz(path, members)
    if timings is not None:
        timings.update(write=time.perf_counter() - t0)

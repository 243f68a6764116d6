"""`np.savez_compressed` for mappings that mix host arrays and device tensors, and the rule that says who compresses: the one writer of the
Moving-MNIST test-set file (preprocessing/mnist/make_test_set.py) and of the evaluation scripts' result files (test/mnist/test.py,
test/utils.run_content_swap).

Who compresses: the environment variable VARSEP_NPZ_COMPRESS=host|device (`compress=` in code; the keyword wins, then the variable, then
the default `host`).  `host` downloads every tensor and calls np.savez_compressed: the call and the bytes of the time before the device
encoder existed.  `device` compresses every device tensor in HBM (ops.deflate_raw_slabs: csrc/vs_deflate.hip, run matching + dynamic
Huffman codes per 32 KiB chunk; ops.crc32), downloads only the compressed bytes, lets host zlib compress the host arrays (the small float
files), and writes all members into one zip container (utils/npz.py, which stays host-only); np.load reads either file to the same arrays.
"""
import os
import time
import zlib

import numpy as np
import torch

from .. import ops
from . import npz

COMPRESS_ENV = 'VARSEP_NPZ_COMPRESS'


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


def device_member(name, t, slab_bytes=None):
    """The npz.Member of a device tensor (made contiguous): its pieces are compressed on the device one slab of `slab_bytes` of input at
    a time as the writer consumes them, and only the compressed bytes are downloaded; its CRC is computed on the device."""
    t = t.contiguous()
    header = npz.npy_header(tuple(t.shape), npz.numpy_dtype(t.dtype))
    return npz.Member(name + '.npy', header, (piece.cpu().numpy() for piece, _ in ops.deflate_raw_slabs(t, slab_bytes=slab_bytes)),
                      ops.crc32(t, init=zlib.crc32(header)), t.numel() * t.element_size())


def savez_compressed(path, arrays, compress=None, timings=None, slab_bytes=None):
    """Writes `arrays` (an ordered mapping of name -> NumPy array or tensor) to the .npz file `path`, members in the mapping's order.
    compress: 'host' (tensors are downloaded; np.savez_compressed(path, **arrays)), 'device' (every device tensor is a `device_member`,
    every host array and CPU tensor an npz.host_member; one npz.write_npz) or None (`npz_compressor`).  timings: optional dict that
    receives the seconds of 'download' + 'write' (host) or of 'write' (device: compression, download of the compressed bytes and file
    together).  slab_bytes: input bytes per compression pass of the device route (default ops.DEFLATE_SLAB_BYTES)."""
    compress = npz_compressor(compress)
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
            members.append(device_member(name, v, slab_bytes))
        else:
            members.append(npz.host_member(name, v.numpy() if isinstance(v, torch.Tensor) else v))
    if isinstance(path, str) and not path.endswith('.npz'):               # as np.savez does
        path = path + '.npz'
    npz.write_npz(path, members)
    if timings is not None:
        timings.update(write=time.perf_counter() - t0)

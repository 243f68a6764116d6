"""`np.load` of an .npz file into device tensors, and the rule that says who decompresses: the counterpart of utils/savez.py, used by
`MovingMNIST.make_dataset(train=False)` (the test videos of `test/mnist/test.py` and of the content-swap scripts).

Who decompresses: the environment variable VARSEP_NPZ_LOAD=host|device (`load=` in code; the keyword wins, then the variable, then the
default `host`).  `host` is np.load on the host followed by an upload of the decoded arrays: the behaviour of the time before the device
reader existed.  `device` uploads a member's COMPRESSED bytes and inflates them in HBM (ops.inflate_raw: csrc/vs_inflate_chunks.hip, one
wave per segment between two sync markers; ops.crc32 checks the result against the zip record), which works for every member whose
stream is cut at sync markers at most 32 KiB of data apart -- all that this package's device encoder writes -- and for small foreign
members that are one segment.  A member the device route does not cover takes the host route, alone: Fortran-order, object, structured and
big-endian arrays, dtypes torch does not have, and streams that do not chain (a large np.savez_compressed member is one stream without
markers).  Stored members (method 0) are uploaded as they are.  The zip directory and the .npy headers are read by utils/npz.py on the host.

Foreign members: VARSEP_NPZ_FOREIGN=host|device (`foreign=` in code; same precedence, default `host`) matters only while the loader is
`device`.  `host` is the paragraph above.  `device` sends a member that does not chain at sync markers -- every np.savez_compressed member --
to ops.inflate_blocks (csrc/vs_inflate_blocks.hip: block headers found by validation, one wave per span between two of them, each span
decoded twice), and only a member that does not chain there either (more than 1 MiB of input between two block headers the finder knows)
takes the host route.

Which block headers are found: VARSEP_NPZ_FINDER=dynamic|all (`finder=` in code; same precedence, default `dynamic`) matters only while
both rules above say `device`.  `dynamic` finds dynamic-Huffman headers alone, so a member with more than 1 MiB of stored or fixed blocks
between two of them -- random or already-compressed bytes, the noisy parts of float arrays -- goes to the host.  `all` also finds stored
headers (ops.inflate_blocks(stored=True): LEN and NLEN = ~LEN at a byte boundary with zero bits in front; about six candidates per stored
block, all but one false and ignored), which leaves only more than 1 MiB of FIXED blocks between two findable headers (zlib's Z_FIXED) to
the host: the 7-bit fixed header cannot be validated.
"""
import os
import zlib

import numpy as np
import torch

from .. import ops
from . import npz

LOAD_ENV = 'VARSEP_NPZ_LOAD'
FOREIGN_ENV = 'VARSEP_NPZ_FOREIGN'
FINDER_ENV = 'VARSEP_NPZ_FINDER'
_HEAD_BYTES = 1 << 16                # compressed bytes inflated on the host to read a member's .npy header (a header is at most 64 KiB + 10)


def npz_loader(load=None):
    """'host' or 'device': who decompresses an .npz file.  The keyword wins; None reads the environment variable VARSEP_NPZ_LOAD; when that
    is unset or empty the host does (np.load, the behaviour before the device reader existed).  Any other value raises, naming the two."""
    source = 'load'
    if load is None:
        load, source = os.environ.get('VARSEP_NPZ_LOAD', '') or 'host', LOAD_ENV
    if load not in ('host', 'device'):
        raise ValueError("%s=%r: 'host' or 'device' expected" % (source, load))
    return load


def npz_foreign(foreign=None):
    """'host' or 'device': who decompresses a member that is not cut at sync markers while the loader is 'device'.  The keyword wins; None
    reads the environment variable VARSEP_NPZ_FOREIGN; when that is unset or empty the host does (the behaviour before the block-parallel
    reader existed).  Any other value raises, naming the two."""
    source = 'foreign'
    if foreign is None:
        foreign, source = os.environ.get('VARSEP_NPZ_FOREIGN', '') or 'host', FOREIGN_ENV
    if foreign not in ('host', 'device'):
        raise ValueError("%s=%r: 'host' or 'device' expected" % (source, foreign))
    return foreign


def npz_finder(finder=None):
    """'dynamic' or 'all': which block headers the block-parallel reader looks for while the loader and the foreign rule are both 'device'.
    The keyword wins; None reads the environment variable VARSEP_NPZ_FINDER; when that is unset or empty dynamic-Huffman headers alone are
    found (the behaviour before the stored finder existed).  Any other value raises, naming the two."""
    source = 'finder'
    if finder is None:
        finder, source = os.environ.get('VARSEP_NPZ_FINDER', '') or 'dynamic', FINDER_ENV
    if finder not in ('dynamic', 'all'):
        raise ValueError("%s=%r: 'dynamic' or 'all' expected" % (source, finder))
    return finder


def _key(entry):
    return entry.name[:-4] if entry.name.endswith('.npy') else entry.name


def _upload(array, device):
    """A host array as a device tensor; what torch cannot hold (object, structured arrays, dtypes it lacks) stays the host array."""
    array = np.asarray(array)
    if array.dtype.hasobject or array.dtype.fields is not None:
        return array
    if array.dtype.byteorder == '>':
        array = array.astype(array.dtype.newbyteorder('='))
    try:
        return torch.from_numpy(np.ascontiguousarray(array).reshape(array.shape)).to(device)
    except TypeError:
        return array


def _device_cover(header):
    """None when the device route covers an array of this header, else why not."""
    dt = header.dtype
    if header.fortran_order:
        return 'Fortran order'
    if dt.hasobject:
        return 'object array'
    if dt.fields is not None or dt.subdtype is not None:
        return 'structured dtype'
    if dt.byteorder == '>':
        return 'big-endian'
    try:
        torch.from_numpy(np.empty((0,), dtype=dt))
    except TypeError:
        return 'dtype %s is not a torch dtype' % dt
    return None


def _member_header(path, entry):
    """The NpyHeader of a member, from the first bytes of its data alone (inflated by host zlib when the member is deflated)."""
    with open(path, 'rb') as f:
        f.seek(entry.data_offset)
        head = f.read(min(entry.csize, _HEAD_BYTES))
    if entry.method == 8:
        head = zlib.decompressobj(-15).decompress(head, _HEAD_BYTES + 16)
    return npz.parse_npy_header(head)


def _as_array(raw, header):
    """uint8 [usize] on the device (header + data) -> the array as a tensor of the header's dtype and shape."""
    dtype = torch.from_numpy(np.empty((0,), dtype=header.dtype)).dtype
    data = raw[header.header_bytes:]
    count = int(np.prod(header.shape, dtype=np.int64))
    if data.numel() != count * header.dtype.itemsize:
        raise ValueError('%d bytes of data for an array of shape %s and dtype %s' % (data.numel(), header.shape, header.dtype))
    if data.numel() and data.data_ptr() % header.dtype.itemsize:
        data = data.clone()                                                 # a header that is no multiple of the item size (old writers)
    return data.view(dtype).reshape(header.shape)


def load(path, device, keys=None, load=None, report=None, foreign=None, finder=None):
    """The arrays of the .npz file `path` as {name: tensor on `device`}, names as np.load gives them; keys: the names wanted (default
    all, in the file's order).  load: 'host' (np.load, then an upload), 'device' (see the module docstring) or None (`npz_loader`).
    report: optional dict that receives name -> (route, why) with route 'host', 'device' or 'stored'.  An array torch cannot hold (object,
    structured) is returned as the host array.  A damaged member raises what np.load raises for it (zipfile.BadZipFile, zlib.error, ...).
    foreign: 'host', 'device' or None (`npz_foreign`): with load='device', who decompresses a member that does not chain at sync markers.
    finder: 'dynamic', 'all' or None (`npz_finder`): with both 'device', whether stored block headers are found too."""
    load = npz_loader(load)
    foreign = npz_foreign(foreign)
    finder = npz_finder(finder)
    device = torch.device(device)
    report = {} if report is None else report
    out = {}
    if load == 'host':
        with np.load(path, allow_pickle=True) as z:
            for name in (z.files if keys is None else keys):
                out[name] = _upload(z[name], device)
                report[name] = ('host', 'load=host')
        return out
    entries = {_key(e): e for e in npz.read_directory(path)}
    host_file = None
    try:
        for name in (list(entries) if keys is None else keys):
            if name not in entries:
                raise KeyError('%s is not a file in the archive' % name)
            e = entries[name]
            why, header = None, None
            if not e.name.endswith('.npy'):
                why = 'not an array'
            else:
                try:
                    header = _member_header(path, e)
                    why = _device_cover(header)
                except Exception as exc:                                    # a damaged start: np.load says what is wrong with it
                    why = 'header: %s' % exc
            if why is None:
                comp = torch.from_numpy(np.fromfile(path, dtype=np.uint8, count=e.csize, offset=e.data_offset)).to(device)
                if e.method == 0:
                    if ops.crc32(comp) != e.crc32:
                        import zipfile
                        raise zipfile.BadZipFile('Bad CRC-32 for file %r' % e.name)
                    raw, route = comp, ('stored', 'method 0')
                else:
                    raw = ops.inflate_raw(comp, e.usize, crc=e.crc32)
                    route = ('device', 'chained at its sync markers')
                    if isinstance(raw, ops.InflateNotChunked) and foreign == 'device':
                        raw = ops.inflate_blocks(comp, e.usize, crc=e.crc32, stored=True) if finder == 'all' \
                            else ops.inflate_blocks(comp, e.usize, crc=e.crc32)
                        route = ('device', 'chained at its block headers')
                    if isinstance(raw, ops.InflateNotChunked):
                        why = 'not chunked: ' + raw.reason
                if why is None:
                    out[name] = _as_array(raw, header)
                    report[name] = route
                    continue
            if host_file is None:
                host_file = np.load(path, allow_pickle=True)
            out[name] = _upload(host_file[name], device)
            report[name] = ('host', why)
    finally:
        if host_file is not None:
            host_file.close()
    return out

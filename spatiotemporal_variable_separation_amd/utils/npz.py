"""An .npz writer that takes members compressed by someone else: the zip container of `np.savez_compressed` (method 8, the names and the
order of np.savez) around raw DEFLATE pieces that the caller supplies -- the device encoder of ops.deflate_raw_slabs in the Moving-MNIST
test-set route, host zlib in the tests.  Host code only: nothing here knows about the GPU.

A member's stream is: its .npy header compressed here by zlib (raw, closed with Z_SYNC_FLUSH: a few hundred bytes on a byte boundary), then
the caller's pieces (each a run of complete non-final blocks that ends on a byte boundary), then the final empty block 03 00.  Its CRC-32
is over header + data, so a producer that computes the data's CRC elsewhere starts it from `zlib.crc32(header)`.  Sizes and the CRC are
written into the local header by seeking back once the pieces are consumed (no data descriptors).  ZIP64 extra fields and end records are
written when a size or an offset needs them (np.savez allows zip64; `--seq_len 250` of the Moving-MNIST test set is a 5.1 GB member), or
always with force_zip64=True.
"""
import io
import struct
import time
import zlib
from collections import namedtuple

import numpy as np

# name: 'sequences.npy'; header: the .npy header bytes (`npy_header`); pieces: iterable of bytes-like compressed pieces of the DATA (the
# header is not among them); crc32: of header + data, an int or a callable evaluated after the pieces are consumed; data_bytes: the
# uncompressed size of the data (without the header)
Member = namedtuple('Member', 'name header pieces crc32 data_bytes')

FINAL_BLOCK = b'\x03\x00'            # BFINAL = 1, fixed codes, end of block
_LIMIT = 0xFFFFFFFF
_ZIP64_FROM = 0xF0000000             # a member this large gets ZIP64 fields up front: its compressed size is unknown until it is written,
#                                      and a stored-only stream is at most 1 % longer than its data (10 bytes per chunk of >= 1 KiB)


def npy_header(shape, dtype):
    """The bytes in front of an array's data in a .npy file (C order), from numpy's own header writer."""
    f = io.BytesIO()
    np.lib.format.write_array_header_1_0(f, {'descr': np.lib.format.dtype_to_descr(np.dtype(dtype)), 'fortran_order': False,
                                             'shape': tuple(int(s) for s in shape)})
    return f.getvalue()


def numpy_dtype(torch_dtype):
    """np.dtype of a torch dtype (through an empty tensor: no table to keep)."""
    import torch
    return torch.empty((0,), dtype=torch_dtype).numpy().dtype


def host_member(name, array, level=6, piece_bytes=1 << 20):
    """A Member whose pieces host zlib makes, `piece_bytes` of data at a time, each closed with a sync flush (what a device producer's
    chunks look like to the writer)."""
    array = np.asarray(array)
    header = npy_header(array.shape, array.dtype)                          # (ascontiguousarray would make a 0-d array 1-d)
    data = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
    state = {'crc': zlib.crc32(header)}

    def pieces():
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        for lo in range(0, data.size, piece_bytes):
            part = data[lo:lo + piece_bytes]
            state['crc'] = zlib.crc32(part, state['crc'])
            yield co.compress(part) + co.flush(zlib.Z_SYNC_FLUSH)

    return Member(name if name.endswith('.npy') else name + '.npy', header, pieces(), lambda: state['crc'], data.size)


def _dos_time():
    t = time.localtime()
    year = max(t.tm_year, 1980)
    return (t.tm_hour << 11) | (t.tm_min << 5) | (t.tm_sec // 2), ((year - 1980) << 9) | (t.tm_mon << 5) | t.tm_mday


def _local_header(name, crc, csize, usize, zip64, dos):
    extra = struct.pack('<HHQQ', 1, 16, usize, csize) if zip64 else b''
    if zip64:
        csize = usize = _LIMIT
    return struct.pack('<4sHHHHHIIIHH', b'PK\x03\x04', 45 if zip64 else 20, 0, 8, dos[0], dos[1], crc, csize, usize, len(name), len(extra)) + name + extra


def write_npz(path, members, force_zip64=False):
    """Writes the zip file `path` with `members` (Member tuples) in their order.  Returns [(name, uncompressed bytes, compressed bytes)]."""
    records, dos = [], _dos_time()
    with open(path, 'wb') as f:
        for m in members:
            name = m.name.encode('utf-8')
            usize = len(m.header) + int(m.data_bytes)
            offset = f.tell()
            zip64 = bool(force_zip64) or usize >= _ZIP64_FROM
            f.write(_local_header(name, 0, 0, usize, zip64, dos))
            start = f.tell()
            co = zlib.compressobj(6, zlib.DEFLATED, -15)
            f.write(co.compress(m.header) + co.flush(zlib.Z_SYNC_FLUSH))
            for piece in m.pieces:
                f.write(piece)
            f.write(FINAL_BLOCK)
            end = f.tell()
            csize = end - start
            crc = int(m.crc32() if callable(m.crc32) else m.crc32) & _LIMIT
            if not zip64 and csize >= _LIMIT:
                raise ValueError('%s: %d compressed bytes need ZIP64 fields that were not reserved' % (m.name, csize))
            f.seek(offset)
            f.write(_local_header(name, crc, csize, usize, zip64, dos))
            f.seek(end)
            records.append((name, crc, csize, usize, offset, zip64))
        cd_offset = f.tell()
        for name, crc, csize, usize, offset, zip64 in records:
            wide = zip64 or offset >= _LIMIT
            extra = b''
            if wide:                     # the fields that are all-ones in the record, in the order usize, csize, offset
                extra = struct.pack('<HHQQQ', 1, 24, usize, csize, offset)
                usize = csize = offset = _LIMIT
            f.write(struct.pack('<4sHHHHHHIIIHHHHHII', b'PK\x01\x02', (3 << 8) | (45 if wide else 20), 45 if wide else 20, 0, 8, dos[0], dos[1], crc,
                                csize, usize, len(name), len(extra), 0, 0, 0, 0o600 << 16, offset) + name + extra)
        cd_size = f.tell() - cd_offset
        count = len(records)
        if force_zip64 or count >= 0xFFFF or cd_offset >= _LIMIT or cd_size >= _LIMIT:
            f.write(struct.pack('<4sQHHIIQQQQ', b'PK\x06\x06', 44, 45, 45, 0, 0, count, count, cd_size, cd_offset))
            f.write(struct.pack('<4sIQI', b'PK\x06\x07', 0, cd_offset + cd_size, 1))
            count, cd_size, cd_offset = min(count, 0xFFFF), min(cd_size, _LIMIT), min(cd_offset, _LIMIT)
            if force_zip64:
                count, cd_size, cd_offset = 0xFFFF, _LIMIT, _LIMIT
        f.write(struct.pack('<4sHHHHIIH', b'PK\x05\x06', 0, 0, count, count, cd_size, cd_offset, 0))
    return [(name.decode('utf-8'), usize, csize) for name, _, csize, usize, _, _ in records]

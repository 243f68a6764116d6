"""An .npz writer that takes members compressed by someone else: the zip container of `np.savez_compressed` (method 8, the names and the
order of np.savez) around raw DEFLATE pieces that the caller supplies -- the device encoder of ops.deflate_raw_slabs in the Moving-MNIST
test-set route, host zlib in the tests.  Host code only: nothing here knows about the GPU.

A member's stream is: its .npy header compressed here by zlib (raw, closed with Z_SYNC_FLUSH: a few hundred bytes on a byte boundary), then
the caller's pieces (each a run of complete non-final blocks that ends on a byte boundary), then the final empty block 03 00.  Its CRC-32
is over header + data, so a producer that computes the data's CRC elsewhere starts it from `zlib.crc32(header)`.  Sizes and the CRC are
written into the local header by seeking back once the pieces are consumed (no data descriptors).  ZIP64 extra fields and end records are
written when a size or an offset needs them (np.savez allows zip64; `--seq_len 250` of the Moving-MNIST test set is a 5.1 GB member), or
always with force_zip64=True.

The reader's half, host-only as well: `read_directory` lists a file's members from its central directory (methods 0 and 8, the ZIP64
fields above) with the offset of each member's data, and `parse_npy_header` reads the .npy 1.0 / 2.0 header in front of an array's bytes.
utils/loadz.py decides from them which members the device decodes.
"""
import io
import struct
import time
import zipfile
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


# ---- reading ------------------------------------------------------------------------------------------------------------------------
# name: as in the archive ('sequences.npy'); method: 0 stored, 8 deflated; crc32, csize, usize: of the central record (ZIP64 resolved);
# data_offset: where the member's csize bytes start in the file
Entry = namedtuple('Entry', 'name method crc32 csize usize data_offset')
NpyHeader = namedtuple('NpyHeader', 'shape fortran_order dtype header_bytes')


def _zip64_extra(extra, wanted):
    """The values of the ZIP64 extra field (id 1) for the record fields that are all-ones, in the order of `wanted`."""
    at = 0
    while at + 4 <= len(extra):
        tag, size = struct.unpack_from('<HH', extra, at)
        if tag == 1:
            if size < 8 * len(wanted):
                raise zipfile.BadZipFile('ZIP64 extra field of %d bytes for %d values' % (size, len(wanted)))
            return struct.unpack_from('<%dQ' % len(wanted), extra, at + 4)
        at += 4 + size
    raise zipfile.BadZipFile('a record needs ZIP64 fields that are not there')


def read_directory(path):
    """[Entry] of the zip file `path`, in the order of its central directory.  Covered: methods 0 and 8, ZIP64 end records and extra
    fields; refused (zipfile.BadZipFile): no end record, several disks, encrypted members, a local record that disagrees on the name."""
    out = []
    with open(path, 'rb') as f:
        f.seek(0, 2)
        size = f.tell()
        tail_at = max(0, size - (22 + 65535))
        f.seek(tail_at)
        tail = f.read()
        at = tail.rfind(b'PK\x05\x06')
        if at < 0 or at + 22 > len(tail):
            raise zipfile.BadZipFile('%s: no end-of-central-directory record' % path)
        disk, cd_disk, here, count, cd_size, cd_offset, _ = struct.unpack_from('<HHHHIIH', tail, at + 4)
        if here == 0xFFFF or count == 0xFFFF or cd_size == _LIMIT or cd_offset == _LIMIT:
            loc = tail_at + at - 20
            if loc < 0:
                raise zipfile.BadZipFile('%s: ZIP64 locator missing' % path)
            f.seek(loc)
            sig, _, end64, disks = struct.unpack('<4sIQI', f.read(20))
            if sig != b'PK\x06\x07' or disks != 1:
                raise zipfile.BadZipFile('%s: ZIP64 locator missing or several disks' % path)
            f.seek(end64)
            rec = f.read(56)
            sig, _, _, _, disk, cd_disk, here, count, cd_size, cd_offset = struct.unpack('<4sQHHIIQQQQ', rec)
            if sig != b'PK\x06\x06':
                raise zipfile.BadZipFile('%s: ZIP64 end record missing' % path)
        if disk != 0 or cd_disk != 0 or here != count:
            raise zipfile.BadZipFile('%s: an archive of several disks' % path)
        if cd_offset + cd_size > size:
            raise zipfile.BadZipFile('%s: the central directory leaves the file' % path)
        f.seek(cd_offset)
        cd = f.read(cd_size)
        at = 0
        for _ in range(count):
            if at + 46 > len(cd) or cd[at:at + 4] != b'PK\x01\x02':
                raise zipfile.BadZipFile('%s: bad central record' % path)
            (_, _, flags, method, _, _, crc, csize, usize, n_name, n_extra, n_comment, disk_start, _, _, offset) = \
                struct.unpack_from('<HHHHHHIIIHHHHHII', cd, at + 4)
            name = cd[at + 46:at + 46 + n_name]
            extra = cd[at + 46 + n_name:at + 46 + n_name + n_extra]
            at += 46 + n_name + n_extra + n_comment
            wanted = [k for k, v in (('usize', usize), ('csize', csize), ('offset', offset)) if v == _LIMIT]
            if disk_start == 0xFFFF:
                wanted.append('disk')
            if wanted:
                wide = dict(zip(wanted, _zip64_extra(extra, wanted)))
                usize, csize, offset = wide.get('usize', usize), wide.get('csize', csize), wide.get('offset', offset)
            if flags & 1:
                raise zipfile.BadZipFile('%s: %s is encrypted' % (path, name))
            if method not in (0, 8):
                raise zipfile.BadZipFile('%s: %s uses method %d' % (path, name, method))
            f.seek(offset)
            local = f.read(30)
            if len(local) != 30 or local[:4] != b'PK\x03\x04':
                raise zipfile.BadZipFile('%s: bad local record of %s' % (path, name))
            l_name, l_extra = struct.unpack_from('<HH', local, 26)
            if f.read(l_name) != name:
                raise zipfile.BadZipFile('%s: the local record of %s has another name' % (path, name))
            data_offset = offset + 30 + l_name + l_extra
            if data_offset + csize > size:
                raise zipfile.BadZipFile('%s: %s leaves the file' % (path, name))
            out.append(Entry(name.decode('utf-8' if flags & 0x800 else 'cp437'), method, crc, csize, usize, data_offset))
    return out


def parse_npy_header(raw):
    """NpyHeader of the first bytes of a .npy file (versions 1.0 and 2.0; `raw` holds at least the header): numpy's own header readers.
    ValueError for anything else."""
    f = io.BytesIO(bytes(raw))
    version = np.lib.format.read_magic(f)
    if version == (1, 0):
        shape, fortran, dtype = np.lib.format.read_array_header_1_0(f)
    elif version == (2, 0):
        shape, fortran, dtype = np.lib.format.read_array_header_2_0(f)
    else:
        raise ValueError('.npy version %s' % (version,))
    return NpyHeader(tuple(int(v) for v in shape), bool(fortran), dtype, f.tell())

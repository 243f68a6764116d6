"""Inputs of the WINDOW matcher's tests (tests/test_deflate_window_cpu.py, tests/test_deflate_window_gpu.py), rebuilt from seeds, on top of
tests/deflate_inputs.py: small named arrays that each exercise one thing a window search can get wrong, the video-major Moving-MNIST
bytes, the host build of csrc/vs_deflate_window_core.h, and a small inflater that returns the TOKENS of a stream, so that a test can say
what the encoder did and not only that zlib reads it."""
import functools
import struct
import subprocess

import numpy as np

import deflate_inputs as D
import host_build

L = D.L
W = 32768                                                            # DEFLATE's window = VS_DEFLATE_MAX_HISTORY
WINDOW_FIXED, WINDOW_DYNAMIC = 5, 6                                  # the host check's form codes of a chunk written from the window parse
FAR_LENGTHS = (3, 4, 257, 258, 259)
SMALL_DISTANCES = (2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49)             # the first distance of the symbols 1 .. 11
LARGE_DISTANCES = (65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)   # symbols 12 .. 29
FIB_PERIODS = (65, 100, 130, 195, 260, 385, 515, 770)                # symbols 12 .. 19: periods of 5-byte units
FIB_FAR = (1025, 1540, 2050, 3075, 4100, 6145, 8195, 12290, 16385)   # symbols 20 .. 28: sources in the chunk before
HISTORY_OFFSETS = (1, 100, 4096)                                     # arrays compressed from an offset: history shorter than the window


def _rs(seed):
    return np.random.RandomState(seed)


def _fresh(rs, n):
    """n random bytes (no structure to match)."""
    return rs.randint(0, 256, size=n).astype(np.uint8)


def _run_filler(n, first=1):
    """n bytes of runs of 200 equal bytes: filler whose positions are (nearly all) inside runs, which the search does not enter."""
    return ((np.arange(n) // 200) % 199 + first).astype(np.uint8)


def dist_32768():
    """A 300-byte block A at 0 and again at 32768 (distance exactly 32768: the first byte of chunk 1 against the first of its history), a
    block B at 1000 and again at 1000 + 32769 (one byte too far: must not be used)."""
    rs = _rs(901)
    a = _run_filler(2 * L + 2000)
    A, B = _fresh(rs, 300), _fresh(rs, 300)
    a[0:300] = A
    a[W:W + 300] = A
    a[1000:1300] = B
    a[1000 + W + 1:1300 + W + 1] = B
    return a


def history_cut():
    """A 500-byte block at 33000 and again at 65336: the copy's first 200 bytes end chunk 1 (the match is cut there), its last 300 open
    chunk 2 with their source in the history."""
    rs = _rs(902)
    a = _run_filler(3 * L)
    A = _fresh(rs, 500)
    a[33000:33500] = A
    a[65336:65836] = A
    return a


def periods():
    """Period 2 and period 3 patterns: self-overlapping matches (distance below length)."""
    rs = _rs(903)
    return np.concatenate([np.tile(np.array([97, 98], np.uint8), 500), _fresh(rs, 50), np.tile(np.array([120, 121, 122], np.uint8), 400), _fresh(rs, 20)])


def far_lengths():
    """Repeats of exactly 3, 4, 257, 258 and 259 bytes about 6000 bytes behind their source, the bytes round each copy different from those
    round its source.  -> (array, {length: position of the copy})."""
    rs = _rs(904)
    a = _run_filler(12000)
    at, where = 100, {}
    for n in FAR_LENGTHS:
        s = _fresh(rs, n + 2)
        a[at:at + n + 2] = s
        copy = at + 6000
        a[copy:copy + n + 2] = s
        a[copy] = (int(s[0]) + 1) & 255
        a[copy + n + 1] = (int(s[n + 1]) + 1) & 255
        where[n] = copy + 1
        at += n + 2 + 250
    return a, where


def all_distance_symbols():
    """Two chunks; the second uses all 30 distance symbols: runs (distance 1), periodic patterns of the small distances, 12-byte copies from
    exactly the large ones."""
    rs = _rs(905)
    a = np.concatenate([_fresh(rs, L), _run_filler(L)])
    at = L + 64
    a[at:at + 3200] = _fresh(rs, 3200)                                     # what the copies from below 3200 bytes back take; the others
    at += 3200                                                             # take bytes of the chunk before
    for d in LARGE_DISTANCES:
        a[at:at + 3] = _fresh(rs, 3)
        a[at + 3:at + 15] = a[at + 3 - d:at + 15 - d]
        a[at + 15] = (int(a[at + 15 - d]) + 1) & 255
        at += 16
    at += 64
    for d in SMALL_DISTANCES:
        pattern = rs.permutation(256)[:d].astype(np.uint8)
        a[at:at + 192] = np.tile(pattern, 192 // d + 1)[:192]
        at += 192 + 7
    return a


def one_distance_symbol():
    """Random bytes with 20-byte repeats, all at distances 1100 .. 1400 (one symbol), and no run."""
    rs = _rs(906)
    a = _fresh(rs, 6000)
    for k in range(12):
        at = 2000 + 300 * k
        d = 1100 + 25 * k
        a[at:at + 20] = a[at - d:at - d + 20]
        a[at + 20] = (int(a[at - d + 20]) + 1) & 255
    while np.any(a[1:] == a[:-1]):
        eq = np.nonzero(a[1:] == a[:-1])[0] + 1
        a[eq] = (a[eq].astype(np.int64) + 101) & 255
    return a


def _slot(b):
    """The slot of the search's table (csrc/vs_deflate_window_core.h: VSW_HASH_BITS = 14) that the 4 bytes b fall into."""
    v = int(b[0]) | int(b[1]) << 8 | int(b[2]) << 16 | int(b[3]) << 24
    return ((v * 2654435761) & 0xFFFFFFFF) >> 18


def _groups(rs, n, taken):
    """n groups of 4 random bytes in n slots of the table that nothing in `taken` uses; `taken` grows by them."""
    out = []
    while len(out) < n:
        g = _fresh(rs, 4)
        if _slot(g) not in taken:
            taken.add(_slot(g))
            out.append(g)
    return out


def _separator(a, at, nxt, taken, used):
    """a[at]: a byte not in `used` such that none of the 4-byte windows that hold it (the 3 bytes before it, the bytes `nxt` behind it)
    falls into a slot of `taken`: such a window would push a group out of the table before its repeat looks it up."""
    for s in range(256):
        if s in used:
            continue
        around = np.concatenate([a[at - 3:at], np.array([s], np.uint8), nxt[:3]])
        if all(_slot(around[k:k + 4]) not in taken for k in range(len(around) - 3)):
            a[at] = s
            used.add(s)
            return
    raise AssertionError('no separator left')


def fibonacci_distances():
    """Two chunks; the second holds 4180 matches of length 4 whose distance symbols 12 .. 28 have the Fibonacci counts 1597, 987, ... 2, 1,
    1, so that the unrestricted distance tree is 16 deep and the Kraft repair runs on the distance code.  A unit is 4 kept bytes (a group)
    and 1 separator that differs from repeat to repeat.  Near symbols: a pattern of period d = 5 * units; far symbols: units copied from
    islands in the chunk before, which is otherwise one run.  Fibonacci counts leave no slack (the sum of the k smallest is the (k + 2)-th
    minus 1), so no match may be lost: groups get table slots of their own and separators are chosen so that no window round them takes
    such a slot (_slot models the table)."""
    rs = _rs(907)
    fib = [1, 1]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    counts = fib[::-1]                                                     # symbol 12 gets 1597
    a = np.full(2 * L, 7, np.uint8)
    at = L
    taken = set()
    far = [(d, g) for d, c in zip(FIB_FAR, counts[len(FIB_PERIODS):]) for g in _groups(rs, c, taken)]
    for k, (d, g) in enumerate(far):
        nxt = far[k + 1][1] if k + 1 < len(far) else np.zeros(3, np.uint8)
        for where in (at - d, at):                                         # the island, then its repeat
            a[where:where + 4] = g
        a[at + 5:at + 8] = nxt[:3]
        used = set()
        _separator(a, at - d + 4, np.full(3, 7, np.uint8) if k + 1 == len(far) or far[k + 1][0] != d else nxt, taken, used)
        _separator(a, at + 4, nxt, taken, used)
        at += 5
    a[at:at + 3] = (250, 0, 250)
    at += 3
    for d, c in zip(FIB_PERIODS, counts):
        units = d // 5
        taken = set()
        groups = _groups(rs, units, taken)
        used = [set() for _ in range(units)]
        used[units - 1].add(int(a[at - 1]))                                # the byte before the pattern is no separator of its last unit
        done, r = 0, 0
        while done < c:
            for u in range(units):
                if r and done >= c:
                    break
                a[at:at + 4] = groups[u]
                last = r and done + 1 >= c
                _separator(a, at + 4, np.zeros(3, np.uint8) if last else groups[(u + 1) % units], taken, used[u])
                done += 1 if r else 0
                at += 5
            r += 1
        a[at:at + 3] = (units, 0, units)                                   # between two patterns: bytes no other border has
        at += 3
    assert at <= 2 * L, at
    return a[:at].copy()


def hash_collisions():
    """Groups of 4 bytes with the same hash of the search's table but different bytes, between repeats that do match."""
    rs = _rs(908)
    bits, seen, pairs = 14, {}, []
    v = rs.randint(0, 1 << 32, size=400000, dtype=np.uint64)
    h = ((v * 2654435761) & 0xFFFFFFFF) >> (32 - bits)
    for value, slot in zip(v.tolist(), h.tolist()):
        if slot in seen and seen[slot] != value:
            pairs.append((seen[slot], value))
            if len(pairs) == 40:
                break
        seen.setdefault(slot, value)
    parts = []
    for k, (p, q) in enumerate(pairs):
        parts += [np.frombuffer(struct.pack('<I', p), np.uint8), _fresh(rs, 70), np.frombuffer(struct.pack('<I', q), np.uint8), _fresh(rs, 70)]
    a = np.concatenate(parts)
    return np.concatenate([a, _fresh(rs, 100), a[:2000]])


def frame_stride(stride, frames=6, seed=909):
    """`frames` frames of `stride` bytes, each the one before with 3 % of its bytes changed: a stride that is no multiple of 64."""
    rs = _rs(seed + stride)
    f = (rs.randint(0, 4, size=stride) * 60).astype(np.uint8)
    out = []
    for _ in range(frames):
        f = f.copy()
        idx = rs.randint(0, stride, size=stride * 3 // 100)
        f[idx] = rs.randint(0, 256, size=idx.size)
        out.append(f)
    return np.concatenate(out)


def mmnist_video_major():
    """The corpus' Moving-MNIST bytes [T, B, 64, 64] with the videos first, as the evaluation scripts' result files hold them."""
    c = D.MMNIST_CASE
    a = dict(D.corpus())['mmnist'].reshape(c['seq_len'], -1, c['frame'], c['frame'])
    return np.ascontiguousarray(a.swapaxes(0, 1)).reshape(-1)


@functools.lru_cache(maxsize=None)
def inputs():
    """[(name, uint8 array, history)]: `history` bytes at the front of the array are not compressed but lie before the first chunk."""
    out = [('dist_32768', dist_32768(), 0), ('history_cut', history_cut(), 0), ('periods', periods(), 0), ('far_lengths', far_lengths()[0], 0),
           ('all_distance_symbols', all_distance_symbols(), 0), ('one_distance_symbol', one_distance_symbol(), 0),
           ('fibonacci_distances', fibonacci_distances(), 0), ('hash_collisions', hash_collisions(), 0),
           ('stride_4097', frame_stride(4097), 0), ('stride_12288', frame_stride(12288), 0)]
    for off in HISTORY_OFFSETS:
        out.append(('history_%d' % off, frame_stride(5000, frames=4, seed=950), off))
    out.append(('mmnist_video_major', mmnist_video_major(), 0))
    for _, a, _ in out:
        a.setflags(write=False)
    return out


def compile_host_check(tmp_path):
    """tests/host/deflate_window_host_check.cpp.  (exe, sanitized)."""
    return host_build.compile_host_check(tmp_path, 'deflate_window_host_check', start_args=[str(tmp_path / 'empty.out'), str(L)])


def run_host_check(exe, cases, tmp_path, chunk=None, tag='window'):
    """The host build on `cases` = [(array, history)] -> (records, stdout); a record is dict(stream=bytes without the final block,
    n_chunks, forms=[...], sizes=[...], runs_sizes=[...])."""
    chunk = L if chunk is None else chunk
    src, dst = str(tmp_path / (tag + '.bin')), str(tmp_path / (tag + '.out'))
    with open(src, 'wb') as f:
        f.write(struct.pack('<q', len(cases)))
        for a, history in cases:
            f.write(struct.pack('<qq', history, a.size - history) + a.tobytes())
    r = subprocess.run([exe, src, dst, str(chunk)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    blob = open(dst, 'rb').read()
    (count,), at, records = struct.unpack_from('<q', blob, 0), 8, []
    assert count == len(cases)
    for _ in range(count):
        size, n_chunks = struct.unpack_from('<qq', blob, at)
        at += 16
        meta = np.frombuffer(blob, dtype='<i4', count=3 * n_chunks, offset=at).reshape(-1, 3)
        at += 12 * n_chunks
        records.append(dict(stream=blob[at:at + size], n_chunks=n_chunks, forms=meta[:, 0].tolist(), sizes=meta[:, 1].tolist(),
                            runs_sizes=meta[:, 2].tolist()))
        at += size
    assert at == len(blob)
    return records, r.stdout


# ---- a small inflater that keeps the tokens -------------------------------------------------------------------------------------------
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class _Bits:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def take(self, n):
        v = 0
        for k in range(n):
            v |= ((self.data[self.pos >> 3] >> (self.pos & 7)) & 1) << k
            self.pos += 1
        return v


def _decoder(lengths):
    """{(length, code): symbol} of a canonical code."""
    table, code = {}, 0
    for n in range(1, 16):
        for s, ln in enumerate(lengths):
            if ln == n:
                table[(n, code)] = s
                code += 1
        code <<= 1
    return table


def _symbol(bits, table):
    code = 0
    for n in range(1, 16):
        code = (code << 1) | bits.take(1)
        if (n, code) in table:
            return table[(n, code)]
    raise ValueError('no code at bit %d' % bits.pos)


def blocks(stream):
    """The blocks of a raw DEFLATE stream (final block included) as dicts: type 0 / 1 / 2, start (the output position of its first
    byte), tokens [(position, length, distance)] with distance 0 for a literal (stored bytes are no tokens), dist_lengths (dynamic: the
    HDIST code lengths).  No output is built: positions are counted."""
    bits, out, pos = _Bits(stream), [], 0
    while True:
        final, kind = bits.take(1), bits.take(2)
        block = dict(type=kind, start=pos, tokens=[], dist_lengths=None)
        if kind == 0:
            bits.pos = (bits.pos + 7) & ~7
            n = bits.take(16)
            assert bits.take(16) == n ^ 0xFFFF
            bits.pos += 8 * n
            pos += n
        else:
            if kind == 1:
                lit = _decoder([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
                dist = _decoder([5] * 30)
            else:
                assert kind == 2
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[_CL_ORDER[k]] = bits.take(3)
                cl, lengths = _decoder(cl), []
                while len(lengths) < hlit + hdist:
                    s = _symbol(bits, cl)
                    if s < 16:
                        lengths.append(s)
                    elif s == 16:
                        lengths += [lengths[-1]] * (3 + bits.take(2))
                    else:
                        lengths += [0] * (3 + bits.take(3) if s == 17 else 11 + bits.take(7))
                assert len(lengths) == hlit + hdist
                block['dist_lengths'] = lengths[hlit:]
                lit, dist = _decoder(lengths[:hlit]), _decoder(lengths[hlit:])
            while True:
                s = _symbol(bits, lit)
                if s == 256:
                    break
                if s < 256:
                    block['tokens'].append((pos, 1, 0))
                    pos += 1
                    continue
                n = _LEN_BASE[s - 257] + bits.take(_LEN_EXTRA[s - 257])
                d = _symbol(bits, dist)
                d = _DIST_BASE[d] + bits.take(_DIST_EXTRA[d])
                block['tokens'].append((pos, n, d))
                pos += n
        out.append(block)
        if final:
            return out


def matches(stream):
    """[(position, length, distance)] of every match of the stream."""
    return [t for b in blocks(stream) for t in b['tokens'] if t[2]]


def distance_symbol(d):
    return max(k for k, base in enumerate(_DIST_BASE) if base <= d)

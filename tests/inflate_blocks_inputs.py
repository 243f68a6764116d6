"""Inputs of the block-parallel inflater's tests (tests/test_npz_blocks_cpu.py, tests/test_npz_blocks_gpu.py): raw DEFLATE streams of host
zlib alone -- what np.savez_compressed stores, no sync markers -- built at test time with zlib.compressobj(level, DEFLATED, -15, memLevel,
strategy) (a low memLevel closes a block every 128 - 1024 symbols, so a few hundred KB hold hundreds of blocks); a small block walker that
says where the blocks of a stream really start (the truth the finder is compared with: it is not the code under test); and the host build of
csrc/vs_inflate_blocks_core.h (tests/host/inflate_blocks_host_check.cpp), which is the model the kernels are compared with."""
import struct
import subprocess
import zlib

import numpy as np

import deflate_window_inputs as WI
import host_build

WORDS = ('status', 'end', 'final', 'produced', 'externals', 'reach')
WINDOW = 32768
MAX_IN = 1 << 20
CAP_STATUS = 12
PLANTED = 120
_CACHE = {}
_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_DEXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def deflate(data, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return co.compress(bytes(data)) + co.flush()


# ---- the block walker --------------------------------------------------------------------------------------------------------------
def _table(lens):
    """(table, mask): table[next bits, LSB first, & mask] = (symbol << 4) | length of the canonical code with these lengths, 0 for no code."""
    top = max(max(lens), 1)
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for l in range(1, top + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    table = [0] * (1 << top)
    for s, l in enumerate(lens):
        if l:
            rev = int(format(nxt[l], '0%db' % l)[::-1], 2)                  # the code as it stands in the stream, first bit lowest
            nxt[l] += 1
            table[rev::1 << l] = [(s << 4) | l] * (1 << (top - l))
    return table, (1 << top) - 1


_FIXED = (_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _table([5] * 30))


def walk_blocks(comp, stop_bit=None):
    """The blocks of the raw DEFLATE stream `comp`: [dict(start, type, final, header_end, end)] with positions in bits (header_end: behind
    the code lengths of a dynamic block, else start + 3).  A plain RFC 1951 reader, symbol by symbol; raises on a stream that is not one.
    stop_bit: walk only the blocks that start before it (a sample of a long stream)."""
    n = len(comp)
    data = bytes(comp) + bytes(16)
    buf, cnt, p = 0, 0, 0                                                   # bits not yet consumed (LSB first), how many, the next byte

    def bits(k):
        nonlocal buf, cnt, p
        while cnt < k:
            buf |= data[p] << cnt
            p += 1
            cnt += 8
        v = buf & ((1 << k) - 1)
        buf >>= k
        cnt -= k
        return v

    def symbol(code):
        nonlocal buf, cnt, p
        table, mask = code
        if cnt < 16:
            buf |= int.from_bytes(data[p:p + 4], 'little') << cnt
            p += 4
            cnt += 32
        e = table[buf & mask]
        assert e, 'no code'
        buf >>= e & 15
        cnt -= e & 15
        return e >> 4

    blocks = []
    while True:
        start = 8 * p - cnt
        final, btype = bits(1), bits(2)
        header_end = 8 * p - cnt
        if btype == 0:
            bits(cnt & 7)
            length, nlen = bits(16), bits(16)
            assert length ^ 0xFFFF == nlen
            p += length - (cnt >> 3)
            buf, cnt = 0, 0
            assert p <= n
        else:
            assert btype in (1, 2)
            if btype == 1:
                lit, dist = _FIXED
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[_ORDER[i]] = bits(3)
                clt, lens = _table(cl), []
                while len(lens) < hlit + hdist:
                    s = symbol(clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens.extend([lens[-1]] * (3 + bits(2)))
                    elif s == 17:
                        lens.extend([0] * (3 + bits(3)))
                    else:
                        lens.extend([0] * (11 + bits(7)))
                assert len(lens) == hlit + hdist and lens[256]
                lit, dist = _table(lens[:hlit]), _table(lens[hlit:])
                header_end = 8 * p - cnt
            table, mask = lit
            while True:                                                     # the symbols; literals are the hot path
                if cnt < 48:
                    buf |= int.from_bytes(data[p:p + 4], 'little') << cnt
                    p += 4
                    cnt += 32
                e = table[buf & mask]
                assert e, 'no literal/length code'
                buf >>= e & 15
                cnt -= e & 15
                s = e >> 4
                if s < 256:
                    continue
                if s == 256:
                    break
                assert s <= 285
                bits(_LEXTRA[s - 257])
                d = symbol(dist)
                assert d <= 29
                bits(_DEXTRA[d])
        blocks.append(dict(start=start, type=btype, final=final, header_end=header_end, end=8 * p - cnt))
        if final:
            break
        if stop_bit is not None and 8 * p - cnt >= stop_bit:
            return blocks
    assert (8 * p - cnt + 7) // 8 == n, (8 * p - cnt, n)
    return blocks


# ---- the contents --------------------------------------------------------------------------------------------------------------------
def video_major():
    """1.25 MiB of the video-major Moving-MNIST bytes: frames of 4096 bytes, the previous frame of a video 4096 bytes back."""
    return WI.mmnist_video_major()[:40 * WINDOW].tobytes()


def text(n, seed=11):
    """Small-alphabet text: words of a 12-letter alphabet drawn with skewed frequencies."""
    rs = np.random.RandomState(seed)
    words = [bytes(rs.choice(list(b'etaoinshrdlu'), size=rs.randint(2, 9)).astype(np.uint8)) for _ in range(300)]
    p = 1.0 / np.arange(1, 301)
    picks = rs.choice(300, size=n // 4, p=p / p.sum())
    return b' '.join(words[k] for k in picks)[:n]


def period():
    """A random period of 30 000 bytes, 20 times: behind the first period almost every byte is a copy from 30 000 back."""
    return np.random.RandomState(21).randint(0, 256, size=30000).astype(np.uint8).tobytes() * 20


def floats():
    """float32 pieces of different kinds, so that zlib at level 1, memLevel 2 chooses stored, fixed and dynamic blocks in one stream."""
    rs = np.random.RandomState(31)
    pieces = []
    for k in range(12):
        if k % 3 == 0:
            pieces.append(np.sin(np.arange(6000) * 0.01 * (k + 1)).astype(np.float32).tobytes())
        elif k % 3 == 1:
            pieces.append(rs.randint(0, 256, size=9000).astype(np.uint8).tobytes())
        else:
            pieces.append((np.arange(40) % 7).astype(np.float32).tobytes() + np.arange(60, dtype=np.uint8).tobytes())
    return b''.join(pieces)


def two_values():
    rs = np.random.RandomState(41)
    return np.where(rs.randint(0, 64, size=4 << 20) == 0, 200, 3).astype(np.uint8).tobytes()


def planted(header):
    """300 000 random bytes with PLANTED byte-aligned copies of `header` (the bytes of a real dynamic block header, from its first bit).
    Stored (level 0: a compressor would turn the repeated header into matches), the copies stand byte-aligned in the stream, false candidates
    followed by garbage."""
    rs = np.random.RandomState(4242)
    a = rs.randint(0, 256, size=300000).astype(np.uint8)
    h = np.frombuffer(header, np.uint8)
    for at in np.linspace(1000, a.size - 2000, PLANTED).astype(np.int64):
        a[at:at + h.size] = h
    return a.tobytes()


def header_bytes(comp, block):
    """The bits of `block`'s header (from its first bit to behind its code lengths) moved to a byte boundary, zeros behind them."""
    v = int.from_bytes(comp, 'little') >> block['start']
    k = block['header_end'] - block['start']
    return (v & ((1 << k) - 1)).to_bytes((k + 7) // 8, 'little')


def corpus():
    """[dict(name, comp, want, chains: the device route must decode it (no fallback), claims: what test_the_corpus_is_what_it_claims_to_be
    pins, damage: run the truncations and bit flips on it)], built once per process."""
    if 'corpus' in _CACHE:
        return _CACHE['corpus']
    out = []

    def add(name, data, chains=True, damage=False, claims=None, comp=None, **how):
        out.append(dict(name=name, comp=deflate(data, **how) if comp is None else comp, want=bytes(data), chains=chains, damage=damage,
                        claims=claims or {}))

    v = video_major()
    add('video_major_numpy', v, claims=dict(max_blocks=12, min_dynamic=1))                                   # level 6, memLevel 8: what NumPy writes
    add('video_major_mem1', v, mem=1, claims=dict(min_dynamic=50, min_reach=4096))
    t = text(120000)
    for level in (1, 6, 9):
        add('text_mem1_level%d' % level, t, level=level, mem=1, claims=dict(min_dynamic=100, max_mean_produced=2000))
    add('period_30000x20', period(), mem=1, claims=dict(min_dynamic=10, min_external_share=0.9))
    add('floats_level1_mem2', floats(), level=1, mem=2, claims=dict(min_dynamic=3, min_stored=3, min_fixed=1))
    add('zeros_4MiB', bytes(4 << 20), claims=dict(max_blocks=4, min_produced=1 << 20))
    add('two_values_4MiB', two_values(), claims=dict(min_produced=1 << 18))
    rs = np.random.RandomState(51)
    add('random_70000', rs.randint(0, 256, size=70000).astype(np.uint8).tobytes(), claims=dict(only_stored=True))
    add('fixed_below_cap', text(100000, seed=12), strategy=zlib.Z_FIXED, claims=dict(only_fixed=True))
    add('fixed_above_cap', rs.randint(0, 144, size=MAX_IN + 70000).astype(np.uint8).tobytes(), chains=False, strategy=zlib.Z_FIXED,
        claims=dict(only_fixed=True, min_comp=MAX_IN + 1))
    add('empty', b'', claims=dict(blocks=1))
    add('one_byte', b'x', claims=dict(blocks=1))
    add('single_final_block', text(3000, seed=13), damage=True, claims=dict(blocks=1, min_dynamic=1))
    add('text_small_mem1', text(6000, seed=14), mem=1, damage=True, claims=dict(min_dynamic=5))
    add('video_small_mem1', v[:64 * 4096], mem=1, damage=True, claims=dict(min_dynamic=3))
    add('floats_small', floats()[:30000], level=1, mem=2, damage=True, claims=dict(min_stored=1))
    source = out[2]                                                         # a real header from the text stream
    block = [b for b in walk_blocks(source['comp']) if b['type'] == 2 and not b['final']][3]
    header = header_bytes(source['comp'], block)
    add('planted_headers', planted(header), level=0, claims=dict(only_stored=True, planted=header))
    _CACHE['corpus'] = out
    return out


# ---- the host build ------------------------------------------------------------------------------------------------------------------
def compile_host_check(tmp_path):
    """tests/host/inflate_blocks_host_check.cpp.  (exe, sanitized)."""
    return host_build.compile_host_check(tmp_path, 'inflate_blocks_host_check', flags=['-pthread'], start_args=[str(tmp_path / 'empty_ib.out')])


def run_host_check(exe, cases, tmp_path, tag='ib', mode=None, lanes=1):
    """The host build on `cases` = [(comp, want)] -> (records, stdout); a record is dict(cand int64 [n] (bit positions), words int64 [n, 6]
    (WORDS), chain_ok, fail, chain (candidate indices), window_crc int64 [chain + 1], words2 int64 [chain, 3], out bytes).  mode: per case 0,
    or 1 for the truncation and bit-flip runs.  lanes: how many threads play the lanes of the wave."""
    src, dst = str(tmp_path / (tag + '.bin')), str(tmp_path / (tag + '.out'))
    mode = [0] * len(cases) if mode is None else mode
    with open(src, 'wb') as f:
        f.write(struct.pack('<q', len(cases)))
        for (comp, want), m in zip(cases, mode):
            f.write(struct.pack('<qqq', len(comp), len(want), m) + bytes(comp) + bytes(want))
    r = subprocess.run([exe, src, dst, str(lanes)], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    blob = open(dst, 'rb').read()
    (count,), at, records = struct.unpack_from('<q', blob, 0), 8, []
    assert count == len(cases)
    for _ in range(count):
        n_cand, chain_ok, chain_len, produced, fail = struct.unpack_from('<qqqqq', blob, at)
        at += 40
        cand = np.frombuffer(blob, '<i8', n_cand, at)
        at += 8 * n_cand
        words = np.frombuffer(blob, '<i8', 6 * n_cand, at).reshape(n_cand, 6)
        at += 48 * n_cand
        chain = np.frombuffer(blob, '<i8', chain_len, at)
        at += 8 * chain_len
        window_crc = np.frombuffer(blob, '<i8', chain_len + 1, at)
        at += 8 * (chain_len + 1)
        words2 = np.frombuffer(blob, '<i8', 3 * chain_len, at).reshape(chain_len, 3)
        at += 24 * chain_len
        records.append(dict(cand=cand, words=words, chain_ok=bool(chain_ok), fail=fail, chain=chain, window_crc=window_crc, words2=words2,
                            out=blob[at:at + produced]))
        at += produced
    assert at == len(blob)
    return records, r.stdout

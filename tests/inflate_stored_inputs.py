"""Inputs of the stored-block finder's tests (tests/test_npz_stored_cpu.py, tests/test_npz_stored_gpu.py): raw DEFLATE streams of host zlib
in which stored blocks are what matters -- more than the span allowance of incompressible bytes, alone and between two stretches of text,
planted stored headers followed by garbage, empty stored blocks (sync flushes) --, the Python restatement of the candidate rule that the
host build and the kernel are compared with, and the host build of the whole route with both finders
(tests/host/inflate_stored_host_check.cpp, in the record format of inflate_blocks_inputs.run_host_check)."""
import zlib

import numpy as np

import host_build
import inflate_blocks_inputs as IB

MAX_IN = IB.MAX_IN
PLANTED = 120
PLANTED_HEADER = bytes([0x00, 0x00, 0x34, 0x12, 0xcb, 0xed])                  # a zero byte (header bits and padding), a spare one, LEN 0x1234, NLEN
_CACHE = {}


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def stored_boundaries(comp):
    """The byte offsets B with B + 4 <= n, (LEN ^ 0xffff) == NLEN and B + 4 + LEN < n: int64 array, sorted."""
    a = np.frombuffer(bytes(comp), np.uint8).astype(np.int64)
    n = a.size
    if n < 5:
        return np.zeros((0,), np.int64)
    length = a[0:n - 3] | (a[1:n - 2] << 8)
    nlen = a[2:n - 1] | (a[3:n] << 8)
    B = np.arange(n - 3, dtype=np.int64)
    return B[((length ^ 0xffff) == nlen) & (B + 4 + length < n)]


def stored_candidates(comp):
    """The rule, restated: for a stored boundary B and k = 0 .. 7 the bit position q = 8 B - 3 - k is a candidate when q >= 0 and every bit
    from q to 8 B - 1 is zero.  Sorted list of ints; bit by bit, on purpose nothing like the kernel's words."""
    data = bytes(comp)
    out = []
    for B in stored_boundaries(comp).tolist():
        for k in range(8):
            q = 8 * B - 3 - k
            if q < 0 or any((data[p >> 3] >> (p & 7)) & 1 for p in range(q, 8 * B)):
                break                                                       # a one bit at q - or the stream's start - also ends every larger k
            out.append(q)
    return sorted(out)


def union_candidates(comp, dynamic):
    """The list ops.inflate_block_scan(comp, stored=True) returns: `dynamic` (the dynamic finder's, bit 0 in it) and the rule's, sorted."""
    return sorted(set(int(q) for q in dynamic) | set(stored_candidates(comp)))


# ---- the contents --------------------------------------------------------------------------------------------------------------------
def random_bytes(n, seed):
    return np.random.RandomState(seed).randint(0, 256, size=n).astype(np.uint8).tobytes()


def planted():
    """300 000 random bytes with PLANTED byte-aligned copies of PLANTED_HEADER; stored (level 0), so the copies stand byte-aligned in the
    stream: stored boundaries that are none, each with sixteen zero bits in front of it (all eight candidates), followed by garbage."""
    a = np.frombuffer(random_bytes(300000, 4343), np.uint8).copy()
    h = np.frombuffer(PLANTED_HEADER, np.uint8)
    for at in np.linspace(1000, a.size - 6000, PLANTED).astype(np.int64):
        a[at:at + h.size] = h
    return a.tobytes()


def sync_flushed(data, every=200000):
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    parts = [co.compress(data[at:at + every]) + co.flush(zlib.Z_SYNC_FLUSH) for at in range(0, len(data), every)]
    return b''.join(parts) + co.flush()


def corpus():
    """[dict(name, comp, want, dynamic_chains: the dynamic finder's list alone chains it (no span above the allowance), claims)], built once per process."""
    if 'corpus' in _CACHE:
        return _CACHE['corpus']
    out = []

    def add(name, data, comp, dynamic_chains=False, **claims):
        out.append(dict(name=name, comp=comp, want=bytes(data), dynamic_chains=dynamic_chains, claims=claims))

    r = random_bytes(MAX_IN + 70000, 61)
    add('random_above_cap', r, IB.deflate(r, level=6, mem=8), only_stored=True, min_comp=MAX_IN + 1)
    add('random_level0_above_cap', r, IB.deflate(r, level=0), only_stored=True, min_comp=MAX_IN + 1, stored_len=65535)
    t = IB.text(60000, seed=17)
    trt = t + r + t
    add('text_random_text', trt, IB.deflate(trt, level=6), min_dynamic=2, min_gap=MAX_IN + 1)
    p = planted()
    add('planted_stored', p, IB.deflate(p, level=0), dynamic_chains=True, only_stored=True, planted=PLANTED_HEADER)
    s = IB.text(700000, seed=18)
    add('sync_flushed', s, sync_flushed(s), dynamic_chains=True, min_empty_stored=3)
    small = random_bytes(30000, 62)
    add('stored_small', small, IB.deflate(small, level=6), dynamic_chains=True, only_stored=True)
    _CACHE['corpus'] = out
    return out


def damage_cases():
    """[(comp, want)] for the truncation and bit-flip runs: `stored_small`, and the first 200 000 compressed bytes of `text_random_text`
    (its text, the first dynamic headers and the first stored blocks; `want` is what zlib gets out of them, the stream itself does not
    end, so no run of it may chain)."""
    by_name = {c['name']: c for c in corpus()}
    head = by_name['text_random_text']['comp'][:200000]
    return [(by_name['stored_small']['comp'], by_name['stored_small']['want']), (head, zlib.decompressobj(-15).decompress(head))]


# ---- the host build ------------------------------------------------------------------------------------------------------------------
def compile_host_check(tmp_path):
    """tests/host/inflate_stored_host_check.cpp.  (exe, sanitized)."""
    return host_build.compile_host_check(tmp_path, 'inflate_stored_host_check', flags=['-pthread'], start_args=[str(tmp_path / 'empty_is.out')])


def run_host_check(exe, cases, tmp_path, tag='is', mode=None, lanes=1):
    """inflate_blocks_inputs.run_host_check on the stored host build: the same record format, `cand` being the union list.  mode: per case
    0, or 1 for the truncation and bit-flip runs."""
    return IB.run_host_check(exe, cases, tmp_path, tag=tag, mode=mode, lanes=lanes)

"""Inputs of the DEFLATE encoder's tests (tests/test_deflate_cpu.py, tests/test_deflate_gpu.py), rebuilt from seeds; shared so that the host
build of csrc/vs_deflate_core.h and the kernel see the same bytes.  L is the encoder's chunk length, taken from the package."""
import functools
import os
import struct
import subprocess

import numpy as np

import host_build
import mmnist_testset_inputs as MI
import mmnist_testset_ref as MR
from spatiotemporal_variable_separation_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = ops.DEFLATE_CHUNK
RUN_EDGES = (1, 2, 3, 4, 257, 258, 259, 260, 261, 516, 517)         # the length-code edges and the 1- and 2-byte remainders
MMNIST_CASE = dict(images=60, seed=42, seq_len=20, digits=2, frame=64, speed=4, standin_seed=5101)
SOURCE_OFFSET = {'odd_len_off1': 1, 'odd_len_off3': 3}               # bytes between the allocation and the source pointer (GPU test)
FINAL_BLOCK = b'\x03\x00'


def _rand(seed, n, hi=256):
    return np.random.RandomState(seed).randint(0, hi, size=n).astype(np.uint8)


def fibonacci_bytes():
    """21 symbols with counts 1, 1, 2, 3, 5, ... (28 656 bytes), shuffled so that no byte equals its predecessor: no run, and an unrestricted
    Huffman tree 20 deep."""
    counts = [1, 1]
    while len(counts) < 21:
        counts.append(counts[-1] + counts[-2])
    rng = np.random.RandomState(77)
    a = rng.permutation(np.repeat(np.arange(21, dtype=np.uint8) * 11 + 3, counts))
    n = len(a)
    assert n == 28656

    def fits(v, i):
        return (i == 0 or a[i - 1] != v) and (i == n - 1 or a[i + 1] != v)

    for _ in range(20):
        bad = np.nonzero(a[1:] == a[:-1])[0] + 1
        if len(bad) == 0:
            break
        for i in bad:
            if a[i] != a[i - 1]:
                continue
            for j in rng.randint(0, n, size=200):
                if abs(int(j) - int(i)) > 1 and fits(a[j], i) and fits(a[i], j):
                    a[i], a[j] = a[j], a[i]
                    break
    assert not np.any(a[1:] == a[:-1])
    return a


def mmnist_bytes():
    images, labels = MI.standins(MMNIST_CASE)
    c = MMNIST_CASE
    return np.ascontiguousarray(MR.make_test_set(images, labels, c['seed'], c['seq_len'], c['digits'], c['frame'], c['speed'])['sequences']).reshape(-1)


def noisy_probe():
    """A 512 x 512 gradient (x + y) // 8 with +-2 noise: literal-heavy, nothing for a run matcher."""
    y, x = np.mgrid[0:512, 0:512]
    noise = np.random.RandomState(1).randint(-2, 3, size=(512, 512))
    return np.clip((x + y) // 8 + noise, 0, 255).astype(np.uint8).reshape(-1)


@functools.lru_cache(maxsize=None)
def corpus():
    """[(name, uint8 array)]; the arrays are shared and must not be written to."""
    out = [('empty', np.zeros(0, np.uint8)), ('one_byte', np.array([200], np.uint8))]
    for name, n in (('L_minus_1', L - 1), ('L', L), ('L_plus_1', L + 1), ('3L_plus_5', 3 * L + 5)):
        a = _rand(11 + n % 97, n, 7)                                       # a small alphabet: runs and literals
        a[n // 3:n // 3 + min(n // 4, 9000)] = 0
        out.append((name, a))
    for name in SOURCE_OFFSET:
        a = _rand(23, 70001 if name.endswith('1') else 4099, 5)
        out.append((name, a))
    out += [('zeros_chunk', np.zeros(L, np.uint8)), ('zeros_300k', np.zeros(300000, np.uint8))]
    for r in RUN_EDGES:
        out.append(('run_%d' % r, np.array([1, 2] + [9] * r + [3, 4], np.uint8)))
    out.append(('run_edges', np.concatenate([np.array([100 + k] + [9] * r, np.uint8) for k, r in enumerate(RUN_EDGES)] + [np.array([5], np.uint8)])))
    out.append(('random_40000', _rand(31, 40000)))
    out.append(('no_neighbour', (np.arange(L) % 251).astype(np.uint8)))
    out.append(('fibonacci', fibonacci_bytes()))
    out.append(('all_256', np.random.RandomState(41).permutation(np.arange(L) % 256).astype(np.uint8)))
    out.append(('two_values', (_rand(43, L, 2) * 255).astype(np.uint8)))
    out.append(('mmnist', mmnist_bytes()))
    out.append(('noisy_probe', noisy_probe()))
    for _, a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mixtures(count=500):
    """Seeded mixtures of runs and noise, lengths drawn around the chunk length and the run-length edges."""
    out = []
    for k in range(count):
        rs = np.random.RandomState(7000 + k)
        target = int(rs.choice([rs.randint(1, 2000), L - 1, L, L + 1, rs.randint(1, 3 * L)], p=[0.5, 0.1, 0.1, 0.1, 0.2]))
        parts, n = [], 0
        while n < target:
            if rs.rand() < 0.5:
                m = int(rs.choice(list(RUN_EDGES) + [int(rs.randint(1, 600)), int(rs.randint(1, 40000))]))
                parts.append(np.full(m, rs.randint(0, 256), np.uint8))
            else:
                m = int(rs.randint(1, 300))
                parts.append(rs.randint(0, int(rs.choice([2, 3, 20, 256])), size=m).astype(np.uint8))
            n += m
        a = np.concatenate(parts)[:target]
        a.setflags(write=False)
        out.append(a)
    return out


def bound(n, chunk=None):
    """The bound on the whole stream: every chunk is at most its bytes + 5 per stored block of at most 65 535 bytes + 5 of its closing
    marker (the slot size), and the stream ends with the 2 bytes of the final block."""
    chunk = L if chunk is None else chunk
    lens = [min(chunk, n - lo) for lo in range(0, n, chunk)]
    return sum(m + 5 * (-(-m // 65535)) + 5 for m in lens) + 2


def compile_host_check(tmp_path):
    """tests/host/deflate_host_check.cpp.  (exe, sanitized)."""
    return host_build.compile_host_check(tmp_path, 'deflate_host_check', start_args=[str(tmp_path / 'empty.out'), str(L)])


def run_host_check(exe, arrays, tmp_path, chunk=None, tag='corpus'):
    """The host build on `arrays` -> (records, stdout); a record is dict(stream=bytes without the final block, n_chunks, crc=(init 0, init
    0xDEADBEEF), forms=[...], sizes=[...])."""
    chunk = L if chunk is None else chunk
    src, dst = str(tmp_path / (tag + '.bin')), str(tmp_path / (tag + '.out'))
    with open(src, 'wb') as f:
        f.write(struct.pack('<q', len(arrays)))
        for a in arrays:
            f.write(struct.pack('<q', a.size) + a.tobytes())
    r = subprocess.run([exe, src, dst, str(chunk)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    blob = open(dst, 'rb').read()
    (count,), at, records = struct.unpack_from('<q', blob, 0), 8, []
    assert count == len(arrays)
    for _ in range(count):
        size, n_chunks, crc0, crc1 = struct.unpack_from('<qqII', blob, at)
        at += 24
        meta = np.frombuffer(blob, dtype='<i4', count=2 * n_chunks, offset=at).reshape(-1, 2)
        at += 8 * n_chunks
        records.append(dict(stream=blob[at:at + size], n_chunks=n_chunks, crc=(crc0, crc1), forms=meta[:, 0].tolist(), sizes=meta[:, 1].tolist()))
        at += size
    assert at == len(blob)
    return records, r.stdout

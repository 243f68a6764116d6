"""Inputs of the chunk-parallel inflater's tests (tests/test_npz_load_cpu.py, tests/test_npz_load_gpu.py): member streams as utils/npz.py
lays them out -- the .npy header piece of host zlib closed with a sync flush, the encoders' chunks, the final block -- built with the HOST
builds of the two encoders (tests/deflate_inputs.py, tests/deflate_window_inputs.py) so that no GPU is needed, plus foreign streams of
zlib alone; and the host build of csrc/vs_inflate_chunks_core.h (tests/host/inflate_chunks_host_check.cpp), which is the model the kernels
are compared with."""
import struct
import subprocess
import zlib

import numpy as np

import deflate_inputs as D
import deflate_window_inputs as WI
import host_build
from spatiotemporal_variable_separation_amd.utils import npz

L, W = D.L, WI.W
MARKER = b'\x00\x00\xff\xff'
WORDS = ('status', 'end', 'final', 'produced', 'externals', 'reach')
PLANTED = 200
RUNS_NAMES = ('empty', 'one_byte', 'L_plus_1', '3L_plus_5', 'odd_len_off3', 'zeros_chunk', 'random_40000', 'two_values', 'run_edges')
N_MIXTURES = 200
_CACHE = {}


def header_piece(n_bytes):
    """(.npy header of a uint8 [n_bytes] array, its compressed piece as npz.write_npz writes it)."""
    header = npz.npy_header((n_bytes,), np.uint8)
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return header, co.compress(header) + co.flush(zlib.Z_SYNC_FLUSH)


def member(body, data):
    """(stream, bytes it inflates to) of a member whose data chunks are `body`."""
    header, piece = header_piece(len(data))
    return piece + body + npz.FINAL_BLOCK, header + data


def foreign(data, level=6):
    """What np.savez_compressed stores for `data`: one raw stream of zlib, no sync markers on purpose."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return co.compress(data) + co.flush()


def video_major():
    """256 KiB of the video-major Moving-MNIST bytes: frames of 4096 bytes, the previous frame of a video 4096 bytes back."""
    return WI.mmnist_video_major()[:8 * L]


def planted():
    """200 000 random bytes with PLANTED copies of 00 00 FF FF: stored chunks, and false candidates inside them."""
    rs = np.random.RandomState(4242)
    a = rs.randint(0, 256, size=200000).astype(np.uint8)
    for at in rs.choice(np.arange(0, a.size - 8, 8), size=PLANTED, replace=False):
        a[at:at + 4] = (0, 0, 255, 255)
    return a


def corpus(tmp_path):
    """[dict(name, comp, want, device: written by the project's encoders (must chain), chains: whether the chain must be valid)], built
    once per process."""
    if 'corpus' in _CACHE:
        return _CACHE['corpus']
    runs_exe, _ = D.compile_host_check(tmp_path)
    window_exe, _ = WI.compile_host_check(tmp_path)
    named = dict(D.corpus())
    out = []

    def add(name, body, data, device=True, chains=True, raw=False):
        comp, want = (body, data) if raw else member(body, data)
        out.append(dict(name=name, comp=comp, want=want, device=device, chains=chains))

    arrays = [named[n] for n in RUNS_NAMES] + list(D.mixtures(500)[:N_MIXTURES])
    names = list(RUNS_NAMES) + ['mixture_%d' % k for k in range(N_MIXTURES)]
    for chunk in (1024, L):
        records, _ = D.run_host_check(runs_exe, arrays, tmp_path, chunk=chunk, tag='ic_runs_%d' % chunk)
        for name, a, rec in zip(names, arrays, records):
            if chunk == L or not name.startswith('mixture') or a.size < 20000:
                add('runs_%d_%s' % (chunk, name), rec['stream'], a.tobytes())
    v = video_major()
    (rec,), _ = WI.run_host_check(window_exe, [(v, 0)], tmp_path, chunk=1024, tag='ic_window')
    add('window_1024_video_major', rec['stream'], v.tobytes())
    cut = 3 * L                                                              # a slab border: the second call sees the first as history
    (first, second), _ = WI.run_host_check(window_exe, [(v[:cut], 0), (v[cut - W:], W)], tmp_path, chunk=1024, tag='ic_slab')
    add('window_1024_slab_border', first['stream'] + second['stream'], v.tobytes())
    (rec,), _ = WI.run_host_check(window_exe, [(v, 0)], tmp_path, chunk=L, tag='ic_window_L')
    add('window_%d_video_major' % L, rec['stream'], v.tobytes())
    p = planted()
    for chunk in (1024, L):
        (rec,), _ = D.run_host_check(runs_exe, [p], tmp_path, chunk=chunk, tag='ic_planted_%d' % chunk)
        add('planted_%d' % chunk, rec['stream'], p.tobytes())
    small = (np.arange(10000) % 97).astype(np.uint8).tobytes()
    add('foreign_10k', foreign(small), small, device=False, raw=True)
    big = np.random.RandomState(7).randint(0, 4, size=200000).astype(np.uint8).tobytes()
    add('foreign_200k', foreign(big), big, device=False, chains=False, raw=True)
    flushed = zlib.compressobj(6, zlib.DEFLATED, -15)                       # zlib's own full flushes: markers every 20 000 bytes
    body = b''.join(flushed.compress(big[lo:lo + 20000]) + flushed.flush(zlib.Z_FULL_FLUSH) for lo in range(0, len(big), 20000))
    add('foreign_full_flush', body + flushed.flush(), big, device=False, raw=True)
    _CACHE['corpus'] = out
    return out


def compile_host_check(tmp_path):
    """tests/host/inflate_chunks_host_check.cpp.  (exe, sanitized)."""
    return host_build.compile_host_check(tmp_path, 'inflate_chunks_host_check', start_args=[str(tmp_path / 'empty_ic.out')])


def run_host_check(exe, cases, tmp_path, tag='ic', mode=None):
    """The host build on `cases` = [(comp, want)] -> (records, stdout); a record is dict(cand int64 [n], words int64 [n, 6] (WORDS),
    chain_ok, chain (candidate indices), out bytes).  mode: per case 0, or 1 for the truncation and corruption runs."""
    src, dst = str(tmp_path / (tag + '.bin')), str(tmp_path / (tag + '.out'))
    mode = [0] * len(cases) if mode is None else mode
    with open(src, 'wb') as f:
        f.write(struct.pack('<q', len(cases)))
        for (comp, want), m in zip(cases, mode):
            f.write(struct.pack('<qqq', len(comp), len(want), m) + bytes(comp) + bytes(want))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    blob = open(dst, 'rb').read()
    (count,), at, records = struct.unpack_from('<q', blob, 0), 8, []
    assert count == len(cases)
    for _ in range(count):
        n_cand, chain_ok, chain_len, produced = struct.unpack_from('<qqqq', blob, at)
        at += 32
        cand = np.frombuffer(blob, '<i8', n_cand, at)
        at += 8 * n_cand
        words = np.frombuffer(blob, '<i8', 6 * n_cand, at).reshape(n_cand, 6)
        at += 48 * n_cand
        chain = np.frombuffer(blob, '<i8', chain_len, at)
        at += 8 * chain_len
        records.append(dict(cand=cand, words=words, chain_ok=bool(chain_ok), chain=chain, out=blob[at:at + produced]))
        at += produced
    assert at == len(blob)
    return records, r.stdout

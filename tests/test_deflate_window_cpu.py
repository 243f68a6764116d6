"""The WINDOW matcher of the device DEFLATE encoder, the part that needs no GPU: the entry point's declaration and argument checks, the logic
(csrc/vs_deflate_window_core.h) compiled for the host and run on the corpus of tests/deflate_inputs.py, 500 seeded mixtures and the inputs
of tests/deflate_window_inputs.py -- round trips, never larger than the RUNS matcher chunk by chunk, the reach across chunk borders, what
each new input is there to exercise (read from the stream's tokens), the size bars against zlib -- and the rule that selects the matcher."""
import ctypes
import heapq
import os
import re
import zlib

import numpy as np
import pytest
import torch

import deflate_inputs as D
import deflate_window_inputs as WI
from spatiotemporal_variable_separation_amd import _lib, ops
from spatiotemporal_variable_separation_amd.utils import npz, savez

L, W = D.L, WI.W
ENTRY = 'vs_deflate_chunks_window'


def inflate_raw(stream, history=b''):
    """The bytes of a raw DEFLATE stream by zlib, `history` being what the decoder has produced before it."""
    d = zlib.decompressobj(-15, zdict=history) if history else zlib.decompressobj(-15)
    out = d.decompress(stream)
    assert d.eof and not d.unused_data
    return out


def zlib_raw(data, level):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return co.compress(data) + co.flush()


# ---- the entry point ---------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_built():
    header = open(os.path.join(D.ROOT, 'include', 'varsep_hip.h')).read()
    lib = _lib.load_library()
    assert re.search(r'\bint %s\(' % ENTRY, header) and ENTRY in _lib.SIGNATURES and hasattr(lib, ENTRY)
    for macro, value in (('VS_DEFLATE_MAX_HISTORY', ops.DEFLATE_MAX_HISTORY),):
        assert re.search(r'#define %s %d\b' % (macro, value), header), macro
    assert ops.DEFLATE_MAX_HISTORY == W == 32768 and ops.DEFLATE_WINDOW_GROUP_BYTES == 4 * L
    assert re.search(r'#define VS_DEFLATE_WINDOW_GROUP_BYTES \(4 \* VS_DEFLATE_MAX_CHUNK\)', header)


def test_entry_point_refuses_null_pointers_bad_sizes_history_and_workspace():
    lib = _lib.load_library()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    G = ops.DEFLATE_WINDOW_GROUP_BYTES

    def call(src=p, history=0, n=100, chunk=L, slots=p, stride=L + ops.DEFLATE_SLOT_EXTRA, sizes=p, work=p, work_bytes=G):
        return lib.vs_deflate_chunks_window(src, history, n, chunk, slots, stride, sizes, work, work_bytes, None)

    for kwargs in (dict(src=None), dict(slots=None), dict(sizes=None), dict(n=-1), dict(chunk=0), dict(chunk=L + 1),
                   dict(chunk=ops.DEFLATE_MIN_CHUNK - 1), dict(stride=L + ops.DEFLATE_SLOT_EXTRA - 1), dict(stride=0),
                   dict(n=(1 << 31) * ops.DEFLATE_MIN_CHUNK + 1, chunk=ops.DEFLATE_MIN_CHUNK, stride=L + 16),
                   dict(history=-1), dict(history=W + 1), dict(work=None), dict(work_bytes=G - 1), dict(work_bytes=0),
                   dict(work=ctypes.c_void_p(p.value + 2))):
        assert call(**kwargs) == -1, kwargs
        assert ENTRY in lib.vs_last_error().decode(), kwargs
    call(history=W + 7)
    assert str(W + 7) in lib.vs_last_error().decode()
    assert call(n=0) == 0 and call(n=0, history=W) == 0                     # nothing to do, nothing launched


def test_ops_refuse_an_unknown_matcher(monkeypatch):
    for match in ('zlib', None, 'RUNS', ''):
        with pytest.raises(_lib.VarsepHipError, match='match'):
            ops.deflate_raw(torch.zeros(100, dtype=torch.uint8), match=match)
        with pytest.raises(_lib.VarsepHipError, match='match'):
            list(ops.deflate_raw_slabs(torch.zeros(100, dtype=torch.uint8), match=match))
    with pytest.raises(_lib.VarsepHipError):                                # a known matcher: the device check as before
        ops.deflate_raw(torch.zeros(100, dtype=torch.uint8), match='window')
    monkeypatch.setattr(ops, 'require_cuda', lambda *t: None)
    packed, n_chunks = ops.deflate_raw(torch.zeros(0, dtype=torch.uint8), match='window')
    assert packed.numel() == 0 and n_chunks == 0


# ---- the logic on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """Both host builds run once: dict(window={name: (array, history, record)}, corpus=..., mixtures=[...], runs={name: record of the RUNS
    build}, runs_mixtures=[...])."""
    tmp = tmp_path_factory.mktemp('deflate_window_host')
    exe, sanitized = WI.compile_host_check(tmp)
    runs_exe, _ = D.compile_host_check(tmp)
    corpus, mixtures, new = D.corpus(), D.mixtures(500), WI.inputs()
    out = dict(sanitized=sanitized)
    for tag, cases in (('corpus', [(a, 0) for _, a in corpus]), ('mixtures', [(a, 0) for a in mixtures]), ('window', [(a, h) for _, a, h in new])):
        records, stdout = WI.run_host_check(exe, cases, tmp, tag=tag)
        print(tag, 'sanitizers:', sanitized, '|', ' | '.join(stdout.strip().splitlines()[-2:]))
        n_chunks = sum(-(-(a.size - h) // L) for a, h in cases)
        # the program's own checks: the slot bound, never above the runs parse and its bytes when it is kept, the round trip through
        # csrc/vs_inflate_core.h
        assert stdout.strip().splitlines()[-1] == 'records %d chunks %d mismatches 0' % (len(cases), n_chunks), stdout[-3000:]
        out[tag] = records
    runs_corpus, _ = D.run_host_check(runs_exe, [a for _, a in corpus], tmp, tag='runs_corpus')
    runs_mix, _ = D.run_host_check(runs_exe, list(mixtures), tmp, tag='runs_mixtures')
    runs_new, _ = D.run_host_check(runs_exe, [a[h:] for _, a, h in new], tmp, tag='runs_window')
    return dict(sanitized=sanitized, exe=exe, tmp=tmp,
                corpus={name: (a, 0, rec, runs) for (name, a), rec, runs in zip(corpus, out['corpus'], runs_corpus)},
                mixtures=[(a, 0, rec, runs) for a, rec, runs in zip(mixtures, out['mixtures'], runs_mix)],
                window={name: (a, h, rec, runs) for (name, a, h), rec, runs in zip(new, out['window'], runs_new)})


def _all(host):
    return (list(host['corpus'].items()) + [('mixture %d' % i, v) for i, v in enumerate(host['mixtures'])] + list(host['window'].items()))


def test_every_stream_round_trips_through_zlib_and_keeps_the_chunk_contract(host):
    cases = _all(host)
    assert len(cases) == len(D.corpus()) + 500 + len(WI.inputs())
    for name, (a, h, rec, _) in cases:
        data = a.tobytes()
        assert inflate_raw(rec['stream'] + D.FINAL_BLOCK, data[:h]) == data[h:], name
        n = a.size - h
        assert rec['n_chunks'] == -(-n // L) == len(rec['sizes']) and sum(rec['sizes']) == len(rec['stream']), name
        at = 0
        for k, size in enumerate(rec['sizes']):
            assert 5 <= size <= min(L, n - k * L) + ops.DEFLATE_SLOT_EXTRA, (name, k)
            at += size
            assert rec['stream'][at - 4:at] == b'\x00\x00\xff\xff', (name, k)  # every chunk ends with the sync marker
    assert host['corpus']['empty'][2]['stream'] == b''


def test_no_chunk_is_larger_than_the_runs_matcher_makes_it(host):
    for name, (a, h, rec, runs) in _all(host):
        assert rec['runs_sizes'] == runs['sizes'], name                     # what the window build thinks the runs build makes
        assert all(w <= r for w, r in zip(rec['sizes'], runs['sizes'])), name
        if h == 0 and all(f < 4 for f in rec['forms']):
            assert rec['stream'] == runs['stream'], name                    # the runs parse kept everywhere: the runs bytes
    c = host['corpus']
    for name in ('zeros_chunk', 'zeros_300k', 'random_40000', 'all_256'):
        assert c[name][2]['sizes'] == c[name][3]['sizes'] and c[name][2]['stream'] == c[name][3]['stream'], name
    forms = {f for _, (_, _, rec, _) in _all(host) for f in rec['forms']}
    assert forms >= {0, 1, 2, WI.WINDOW_FIXED, WI.WINDOW_DYNAMIC}, forms


@pytest.mark.parametrize('name', ['mmnist_video_major', 'stride_12288', 'history_cut'])
def test_reach_one_call_equals_two_calls_with_history_and_beats_calls_without(host, name):
    a, _, rec, _ = host['window'][name]
    cut = 2 * L if a.size > 2 * L else L
    (first, second, alone), _ = WI.run_host_check(host['exe'], [(a[:cut], 0), (a[cut - W:], W), (a[cut:], 0)], host['tmp'], tag='reach')
    assert first['stream'] + second['stream'] == rec['stream']              # the history of the second call is what the first one saw
    cut_stream = first['stream'] + alone['stream']
    assert inflate_raw(cut_stream + D.FINAL_BLOCK) == a.tobytes()
    assert len(cut_stream) >= len(rec['stream'])
    print(name, 'one call', len(rec['stream']), 'cut without history', len(cut_stream))
    if name == 'mmnist_video_major':
        assert len(cut_stream) > len(rec['stream'])


def test_chunks_without_history_are_strictly_larger_on_the_video_major_bytes(host):
    a, _, rec, _ = host['window']['mmnist_video_major']
    pieces = [(a[lo:lo + L], 0) for lo in range(0, a.size, L)]
    records, _ = WI.run_host_check(host['exe'], pieces, host['tmp'], tag='independent')
    stream = b''.join(r['stream'] for r in records)
    assert inflate_raw(stream + D.FINAL_BLOCK) == a.tobytes()
    print('video-major: with history %d, every chunk alone %d' % (len(rec['stream']), len(stream)))
    assert len(stream) > len(rec['stream'])


def test_smaller_chunks_reach_back_the_same_way(host):
    a, _, _, _ = host['window']['stride_4097']
    for chunk in (1024, 4096):
        (rec,), stdout = WI.run_host_check(host['exe'], [(a, 0)], host['tmp'], chunk=chunk, tag='chunk%d' % chunk)
        assert stdout.strip().splitlines()[-1].endswith('mismatches 0')
        assert inflate_raw(rec['stream'] + D.FINAL_BLOCK) == a.tobytes() and rec['n_chunks'] == -(-a.size // chunk)
        assert any(d > chunk for _, _, d in WI.matches(rec['stream'] + D.FINAL_BLOCK))    # a source before the chunk


# ---- what each new input is there for, read from the tokens ------------------------------------------------------------------------
def _matches(host, name):
    return WI.matches(host['window'][name][2]['stream'] + D.FINAL_BLOCK)


def test_distance_exactly_32768_is_used_and_32769_is_not(host):
    m = _matches(host, 'dist_32768')
    at_border = [t for t in m if t[0] == W]
    assert at_border == [(W, 258, 32768)] and (W + 258, 42, 32768) in m     # the 300 bytes of A, from the first byte of the history
    assert max(d for _, _, d in m) == 32768
    assert not [t for t in m if 1000 + W + 1 <= t[0] < 1300 + W + 1 and t[1] > 4]   # B's only source lies 32769 back


def test_a_match_is_cut_at_the_chunks_end_and_goes_on_from_the_history(host):
    m = _matches(host, 'history_cut')
    d = 65336 - 33000
    assert (65336, 200, d) in m and (2 * L, 258, d) in m and (2 * L + 258, 42, d) in m
    assert all(p // L == (p + n - 1) // L for p, n, _ in m)                 # no match crosses a chunk border


def test_self_overlapping_matches(host):
    m = _matches(host, 'periods')
    assert [t for t in m if t[0] < 1000 and t[2] % 2 == 0 and t[2] < t[1]] and [t for t in m if t[0] > 1050 and t[2] % 3 == 0 and t[2] < t[1]]


def test_lengths_at_a_far_distance(host):
    m = {p: (n, d) for p, n, d in _matches(host, 'far_lengths')}
    where = WI.far_lengths()[1]
    assert where[3] not in m and not [1 for p, (n, d) in m.items() if n == 3 and d > 4096]   # three literals are cheaper
    assert m[where[4]] == (4, 6000) and m[where[257]] == (257, 6000) and m[where[258]] == (258, 6000) and m[where[259]] == (258, 6000)
    assert where[259] + 258 not in m                                        # the 259th byte is a literal


def test_one_block_uses_all_30_distance_symbols(host):
    block = [b for b in WI.blocks(host['window']['all_distance_symbols'][2]['stream'] + D.FINAL_BLOCK) if b['start'] == L and b['tokens']][0]
    assert block['type'] == 2 and len(block['dist_lengths']) == 30 and all(block['dist_lengths'])
    assert {WI.distance_symbol(d) for _, _, d in block['tokens'] if d} == set(range(30))
    assert {d for _, _, d in block['tokens']} >= set(WI.LARGE_DISTANCES) | set(WI.SMALL_DISTANCES) | {1}


def test_a_block_with_exactly_one_distance_symbol(host):
    (block,) = [b for b in WI.blocks(host['window']['one_distance_symbol'][2]['stream'] + D.FINAL_BLOCK) if b['tokens']]
    assert block['type'] == 2 and sorted(set(block['dist_lengths'])) == [0, 1] and block['dist_lengths'].count(1) == 1
    assert len({WI.distance_symbol(d) for _, _, d in block['tokens'] if d}) == 1 and sum(1 for t in block['tokens'] if t[2]) == 12


def _huffman_depth(counts):
    heap = [(c, 0) for c in counts if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return heap[0][1]


def test_fibonacci_distances_drive_the_kraft_repair_of_the_distance_code(host):
    block = [b for b in WI.blocks(host['window']['fibonacci_distances'][2]['stream'] + D.FINAL_BLOCK) if b['start'] == L and b['tokens']][0]
    counts = np.bincount([WI.distance_symbol(d) for _, _, d in block['tokens'] if d], minlength=30)
    print('distance symbol counts', counts.tolist(), 'unrestricted depth', _huffman_depth(counts), 'lengths', block['dist_lengths'])
    assert counts.sum() >= 4100 and _huffman_depth(counts) > 15             # an unrestricted tree would not fit 15 bits
    lengths = block['dist_lengths'] + [0] * (30 - len(block['dist_lengths']))
    assert max(lengths) == 15 and all((n > 0) == (c > 0) for n, c in zip(lengths, counts))
    assert sum(2.0 ** -n for n in lengths if n) == 1.0                      # complete after the repair


def test_hash_collisions_are_verified_and_odd_strides_and_short_histories_match(host):
    a, _, rec, runs = host['window']['hash_collisions']
    m = WI.matches(rec['stream'] + D.FINAL_BLOCK)
    assert m and all(a[p:p + n].tobytes() == a[p - d:p - d + n].tobytes() for p, n, d in m)
    for name, stride in (('stride_4097', 4097), ('stride_12288', 12288)):
        a, _, rec, runs = host['window'][name]
        m = WI.matches(rec['stream'] + D.FINAL_BLOCK)
        at_stride = sum(n for _, n, d in m if d == stride)
        print(name, 'bytes matched one frame back: %d of %d' % (at_stride, a.size))
        assert stride % 64 and at_stride > a.size // 4 or stride == 12288 and at_stride > a.size // 4
        assert len(rec['stream']) < 0.75 * len(runs['stream'])
    for off in WI.HISTORY_OFFSETS:
        a, h, rec, runs = host['window']['history_%d' % off]
        assert h == off and len(rec['stream']) < len(runs['stream'])


# ---- the size bars -----------------------------------------------------------------------------------------------------------------
def test_size_bars_against_zlib_on_the_same_bytes(host):
    a, _, rec, runs = host['window']['mmnist_video_major']
    data = a.tobytes()
    level1, level6 = len(zlib_raw(data, 1)), len(zlib_raw(data, 6))
    ours, runs_bytes = len(rec['stream']) + 2, len(runs['stream']) + 2
    print('video-major Moving-MNIST: window %d bytes, runs %d, zlib level 1 %d, level 6 %d (window / level 1 %.4f, / level 6 %.4f, / runs %.4f)'
          % (ours, runs_bytes, level1, level6, ours / level1, ours / level6, ours / runs_bytes))
    assert ours <= level1 and ours <= 0.5 * runs_bytes
    a, _, rec, runs = host['corpus']['mmnist']
    print('time-major Moving-MNIST: window %d bytes, runs %d' % (len(rec['stream']) + 2, len(runs['stream']) + 2))
    assert len(rec['stream']) <= len(runs['stream'])


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def test_matcher_rule_keyword_over_environment_over_default(monkeypatch):
    assert savez.MATCH_ENV == 'VARSEP_NPZ_MATCH'
    monkeypatch.delenv(savez.MATCH_ENV, raising=False)
    assert savez.npz_matcher() == 'runs' and savez.npz_matcher(None) == 'runs'
    monkeypatch.setenv(savez.MATCH_ENV, '')
    assert savez.npz_matcher() == 'runs'                                    # empty counts as unset
    for env in ('runs', 'window'):
        monkeypatch.setenv(savez.MATCH_ENV, env)
        assert savez.npz_matcher() == env
        for kw in ('runs', 'window'):
            assert savez.npz_matcher(kw) == kw                              # the keyword over the environment
    monkeypatch.setenv(savez.MATCH_ENV, 'lz77')
    with pytest.raises(ValueError, match=r"VARSEP_NPZ_MATCH='lz77'.*'runs' or 'window'"):
        savez.npz_matcher()
    assert savez.npz_matcher('window') == 'window'
    with pytest.raises(ValueError, match=r"match='zlib'.*'runs' or 'window'"):
        savez.npz_matcher('zlib')


class OnDevice(torch.Tensor):
    """A CPU tensor that says it lives on the device."""

    @property
    def is_cuda(self):
        return True

    def cpu(self, *args, **kwargs):
        return self.as_subclass(torch.Tensor)


def _standins(monkeypatch, log, old_signature):
    """ops.deflate_raw_slabs and ops.crc32 by host zlib; with `old_signature` the stand-in does not know the `match` keyword."""
    def pieces(t, slab_bytes):
        data = t.as_subclass(torch.Tensor).reshape(-1).view(torch.uint8).numpy()
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        if data.size:
            yield torch.from_numpy(np.frombuffer(co.compress(data.tobytes()) + co.flush(zlib.Z_SYNC_FLUSH), np.uint8).copy()), 1

    def old(t, chunk_bytes=None, slab_bytes=None):
        log.append(('deflate_raw_slabs', t.numel(), None))
        return pieces(t, slab_bytes)

    def new(t, chunk_bytes=None, slab_bytes=None, match='runs'):
        log.append(('deflate_raw_slabs', t.numel(), match))
        return pieces(t, slab_bytes)

    monkeypatch.setattr(ops, 'deflate_raw_slabs', old if old_signature else new)
    monkeypatch.setattr(ops, 'crc32', lambda t, init=0: zlib.crc32(t.as_subclass(torch.Tensor).reshape(-1).view(torch.uint8).numpy().tobytes(), init))


def test_savez_passes_the_matcher_only_when_asked(monkeypatch, tmp_path):
    frames = torch.from_numpy(np.random.RandomState(5).randint(0, 3, size=(4, 5, 8, 8, 1)).astype(np.uint8)).as_subclass(OnDevice)
    arrays = dict(frames=frames, floats=np.arange(12, dtype=np.float32))
    path = str(tmp_path / 'x.npz')
    monkeypatch.delenv(savez.MATCH_ENV, raising=False)
    log = []
    _standins(monkeypatch, log, old_signature=True)
    savez.savez_compressed(path, arrays, compress='device')                 # nothing said: today's call, a stand-in of the old signature works
    savez.savez_compressed(path, arrays, compress='device', match='runs')
    monkeypatch.setenv(savez.MATCH_ENV, 'runs')
    savez.savez_compressed(path, arrays, compress='device')
    assert log == [('deflate_raw_slabs', frames.numel(), None)] * 3
    with np.load(path) as z:
        assert np.array_equal(z['frames'], frames.cpu().numpy()) and np.array_equal(z['floats'], arrays['floats'])
    del log[:]
    _standins(monkeypatch, log, old_signature=False)
    savez.savez_compressed(path, arrays, compress='device', match='window')
    monkeypatch.setenv(savez.MATCH_ENV, 'window')
    savez.savez_compressed(path, arrays, compress='device')
    savez.savez_compressed(path, arrays, compress='device', match='runs')   # the keyword over the environment
    assert log == [('deflate_raw_slabs', frames.numel(), 'window')] * 2 + [('deflate_raw_slabs', frames.numel(), 'runs')]
    del log[:]
    monkeypatch.setenv(savez.MATCH_ENV, 'both')                             # refused before anything is compressed, on the host route too
    for compress in ('device', 'host'):
        with pytest.raises(ValueError, match='VARSEP_NPZ_MATCH'):
            savez.savez_compressed(path, arrays, compress=compress)
    with pytest.raises(ValueError, match="match='x'"):
        savez.savez_compressed(path, arrays, compress='host', match='x')
    assert log == []

"""DEFLATE compression on the device, the part that needs no GPU: the three entry points' declarations and argument checks, the encoder's
logic (csrc/vs_deflate_core.h) compiled for the host and run on the corpus of tests/deflate_inputs.py plus 500 seeded mixtures, its size
against zlib's on the same bytes, the piecewise CRC-32, the .npz container with host-zlib producers, and the rule that selects who
compresses the Moving-MNIST test file."""
import ctypes
import os
import re
import zipfile
import zlib

import numpy as np
import pytest
import torch

import deflate_inputs as D
import mmnist_testset_inputs as MI
from spatiotemporal_variable_separation_amd import _lib, ops
from spatiotemporal_variable_separation_amd.preprocessing.mnist import make_test_set
from spatiotemporal_variable_separation_amd.utils import npz

ROOT = D.ROOT
ENTRIES = ('vs_deflate_chunks', 'vs_deflate_pack', 'vs_crc32')
STORED, FIXED, DYNAMIC = 0, 1, 2


def inflate_raw(stream):
    """The bytes of a raw DEFLATE stream by zlib; the stream must end with its final block and nothing behind it."""
    d = zlib.decompressobj(-15)
    out = d.decompress(stream)
    assert d.eof and not d.unused_data
    return out


def zlib_raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return co.compress(data) + co.flush()


def test_entry_points_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, 'include', 'varsep_hip.h')).read()
    lib = _lib.load_library()
    for name in ENTRIES:
        assert re.search(r'\bint %s\(' % name, header)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert 'vs_deflate.hip' in _lib.SOURCES
    for macro, value in (('VS_DEFLATE_MAX_CHUNK', ops.DEFLATE_CHUNK), ('VS_DEFLATE_MIN_CHUNK', ops.DEFLATE_MIN_CHUNK),
                         ('VS_DEFLATE_SLOT_EXTRA', ops.DEFLATE_SLOT_EXTRA)):
        assert re.search(r'#define %s %d\b' % (macro, value), header), macro
    assert 16 * 1024 <= D.L <= 64 * 1024 and D.L <= 65535                   # one stored block holds a chunk


def test_entry_points_refuse_null_pointers_and_bad_sizes():
    lib = _lib.load_library()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    L = D.L

    def chunks(src=p, n=100, chunk=L, slots=p, stride=L + ops.DEFLATE_SLOT_EXTRA, sizes=p):
        return lib.vs_deflate_chunks(src, n, chunk, slots, stride, sizes, None)

    def pack(slots=p, stride=L + 16, sizes=p, offsets=p, n=1, dst=p, dst_bytes=64):
        return lib.vs_deflate_pack(slots, stride, sizes, offsets, n, dst, dst_bytes, None)

    def crc(src=p, n=100, chunk=65536, init=0, partial=p):
        return lib.vs_crc32(src, n, chunk, init, partial, None)

    for call, name, bad in (
            (chunks, 'vs_deflate_chunks', [dict(src=None), dict(slots=None), dict(sizes=None), dict(n=-1), dict(chunk=0), dict(chunk=L + 1),
                                           dict(chunk=ops.DEFLATE_MIN_CHUNK - 1), dict(stride=L + ops.DEFLATE_SLOT_EXTRA - 1), dict(stride=0),
                                           dict(n=(1 << 31) * ops.DEFLATE_MIN_CHUNK + 1, chunk=ops.DEFLATE_MIN_CHUNK, stride=L + 16)]),
            (pack, 'vs_deflate_pack', [dict(slots=None), dict(sizes=None), dict(offsets=None), dict(dst=None), dict(n=0), dict(n=-2), dict(stride=0),
                                       dict(dst_bytes=-1), dict(n=1 << 31)]),
            (crc, 'vs_crc32', [dict(src=None), dict(partial=None), dict(n=-1), dict(chunk=255), dict(chunk=(1 << 24) + 1),
                               dict(n=1 << 42, chunk=256)])):
        for kwargs in bad:
            assert call(**kwargs) == -1, (name, kwargs)
            assert name in lib.vs_last_error().decode(), (name, kwargs)
    chunks(stride=L + 9)
    assert str(L + 9) in lib.vs_last_error().decode() and str(ops.DEFLATE_SLOT_EXTRA) in lib.vs_last_error().decode()
    assert chunks(n=0) == 0 and crc(n=0) == 0                               # nothing to do, nothing launched


def test_ops_refuse_cpu_tensors_and_non_contiguous_operands(monkeypatch):
    with pytest.raises(_lib.VarsepHipError):
        ops.deflate_raw(torch.zeros(100, dtype=torch.uint8))
    with pytest.raises(_lib.VarsepHipError):
        list(ops.deflate_raw_slabs(torch.zeros(100, dtype=torch.uint8)))
    with pytest.raises(_lib.VarsepHipError):
        ops.crc32(torch.zeros(100, dtype=torch.uint8))
    monkeypatch.setattr(ops, 'require_cuda', lambda *t: None)               # past the device check, still on the host: nothing is launched
    strided = torch.zeros((8, 8), dtype=torch.uint8)[:, ::2]
    with pytest.raises(_lib.VarsepHipError, match='contiguous'):
        ops.deflate_raw(strided)
    with pytest.raises(_lib.VarsepHipError, match='contiguous'):
        ops.crc32(strided)
    for chunk in (ops.DEFLATE_MIN_CHUNK - 1, D.L + 1):
        with pytest.raises(_lib.VarsepHipError, match='chunk_bytes'):
            ops.deflate_raw(torch.zeros(100, dtype=torch.uint8), chunk_bytes=chunk)
    assert ops.crc32(torch.zeros(0, dtype=torch.uint8), init=77) == 77      # an empty tensor: the CRC is its start value
    packed, n_chunks = ops.deflate_raw(torch.zeros(0, dtype=torch.uint8))
    assert packed.numel() == 0 and n_chunks == 0


# ---- the encoder's logic on the host -----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """The host build run once on the corpus and once on the mixtures: {name: (array, record)}, [(array, record)], sanitized."""
    tmp = tmp_path_factory.mktemp('deflate_host')
    exe, sanitized = D.compile_host_check(tmp)
    out = {}
    for tag, arrays in (('corpus', [a for _, a in D.corpus()]), ('mixtures', D.mixtures(500))):
        records, stdout = D.run_host_check(exe, arrays, tmp, tag=tag)
        print(tag, 'sanitizers:', sanitized, '|', ' | '.join(stdout.strip().splitlines()[-2:]))
        n_chunks = sum(-(-a.size // D.L) for a in arrays)
        # the program's own checks: the slot bound, the smallest form by its own count, the round trip through csrc/vs_inflate_core.h
        assert stdout.strip().splitlines()[-1] == 'records %d chunks %d mismatches 0' % (len(arrays), n_chunks), stdout[-3000:]
        out[tag] = list(zip(arrays, records))
    return dict(corpus={name: pair for (name, _), pair in zip(D.corpus(), out['corpus'])}, mixtures=out['mixtures'], sanitized=sanitized)


def test_corpus_holds_what_the_encoder_can_get_wrong():
    c = dict(D.corpus())
    L = D.L
    assert [c[k].size for k in ('empty', 'one_byte', 'L_minus_1', 'L', 'L_plus_1', '3L_plus_5')] == [0, 1, L - 1, L, L + 1, 3 * L + 5]
    assert all(c[k].size % 4 for k in D.SOURCE_OFFSET) and sorted(D.SOURCE_OFFSET.values()) == [1, 3]
    assert c['zeros_chunk'].size == L and c['zeros_300k'].size == 300000 and not c['zeros_300k'].any()
    assert all('run_%d' % r in c for r in (1, 2, 3, 4, 257, 258, 259, 260, 261, 516, 517))
    assert c['random_40000'].size == 40000 and not np.any(c['no_neighbour'][1:] == c['no_neighbour'][:-1])
    fib = c['fibonacci']
    assert fib.size == 28656 and not np.any(fib[1:] == fib[:-1])
    assert sorted(np.bincount(fib)[np.bincount(fib) > 0].tolist())[:6] == [1, 1, 2, 3, 5, 8] and len(np.unique(fib)) == 21
    counts = np.bincount(c['all_256'], minlength=256)
    assert counts.min() == counts.max() == L // 256 and len(np.unique(c['two_values'])) == 2
    assert c['mmnist'].size == 2457600 and c['noisy_probe'].size == 512 * 512
    assert len(D.mixtures(500)) == 500 and {a.size for a in D.mixtures(500)} >= {L - 1, L, L + 1}


def test_core_on_the_host_round_trips_the_corpus_and_500_mixtures_through_zlib(host):
    pairs = list(host['corpus'].items()) + [('mixture %d' % i, p) for i, p in enumerate(host['mixtures'])]
    assert len(pairs) == len(D.corpus()) + 500
    for name, (a, rec) in pairs:
        data = a.tobytes()
        assert inflate_raw(rec['stream'] + D.FINAL_BLOCK) == data, name
        assert rec['n_chunks'] == -(-a.size // D.L) == len(rec['sizes']) and sum(rec['sizes']) == len(rec['stream']), name
        for k, size in enumerate(rec['sizes']):
            assert size <= min(D.L, a.size - k * D.L) + ops.DEFLATE_SLOT_EXTRA, (name, k)
        assert len(rec['stream']) + len(D.FINAL_BLOCK) <= D.bound(a.size), name
        assert rec['stream'][-4:] == b'\x00\x00\xff\xff' or a.size == 0, name  # every chunk ends with the sync marker
    c = host['corpus']
    assert c['random_40000'][1]['forms'] == [STORED, STORED] and c['all_256'][1]['forms'] == [STORED]
    assert c['fibonacci'][1]['forms'] == [DYNAMIC] and c['no_neighbour'][1]['forms'] == [DYNAMIC]
    assert set(c['mmnist'][1]['forms']) == {DYNAMIC} and c['one_byte'][1]['forms'] == [FIXED]
    assert c['empty'][1]['stream'] == b'' and c['zeros_chunk'][1]['sizes'][0] < 64
    forms = [f for _, (_, rec) in pairs for f in rec['forms']]
    assert {STORED, FIXED, DYNAMIC} == set(forms)


def test_size_bars_against_zlib_on_the_same_bytes(host):
    a, rec = host['corpus']['mmnist']
    level6 = len(zlib_raw(a.tobytes(), 6))
    print('Moving-MNIST set: core %d bytes, zlib level 6 %d (ratio %.4f)' % (len(rec['stream']) + 2, level6, (len(rec['stream']) + 2) / level6))
    assert len(rec['stream']) + 2 <= 1.10 * level6
    a, rec = host['corpus']['noisy_probe']
    huffman = len(zlib_raw(a.tobytes(), 6, zlib.Z_HUFFMAN_ONLY))
    print('noisy probe: core %d bytes, zlib Z_HUFFMAN_ONLY %d (ratio %.4f)' % (len(rec['stream']) + 2, huffman, (len(rec['stream']) + 2) / huffman))
    assert len(rec['stream']) + 2 <= 1.10 * huffman


def test_piecewise_crc_equals_zlib(host):
    seen = set()
    for name, (a, rec) in list(host['corpus'].items()) + [('mixture', p) for p in host['mixtures']]:
        data = a.tobytes()
        assert rec['crc'] == (zlib.crc32(data, 0), zlib.crc32(data, 0xDEADBEEF)), name
        seen.add(a.size)
    assert seen >= {0, 1, D.L - 1, D.L, D.L + 1, 3 * D.L + 5}


# ---- the container -----------------------------------------------------------------------------------------------------------------
def _case_arrays():
    c = MI.CASES['default']
    import mmnist_testset_ref as MR
    images, labels = MI.standins('default')
    return MR.make_test_set(images, labels, c['seed'], c['seq_len'], c['digits'], c['frame'], c['speed'])


@pytest.mark.parametrize('force_zip64', [False, True])
def test_write_npz_with_host_zlib_producers_reads_like_savez_compressed(tmp_path, force_zip64):
    arrays = _case_arrays()
    ref, ours = str(tmp_path / 'ref.npz'), str(tmp_path / 'ours.npz')
    np.savez_compressed(ref, **arrays)
    written = npz.write_npz(ours, [npz.host_member(k, v, piece_bytes=50000) for k, v in arrays.items()], force_zip64=force_zip64)
    with np.load(ref) as want, np.load(ours) as got:
        assert got.files == want.files == list(arrays)
        for k in want.files:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    with zipfile.ZipFile(ref) as zr, zipfile.ZipFile(ours) as zo:
        assert zo.testzip() is None
        assert zo.namelist() == zr.namelist() == [k + '.npy' for k in arrays]
        for a, b in zip(zo.infolist(), zr.infolist()):
            assert (a.compress_type, a.file_size, a.CRC, a.flag_bits) == (zipfile.ZIP_DEFLATED, b.file_size, b.CRC, 0)
            assert a.compress_size < a.file_size
    assert [(n, u) for n, u, _ in written] == [(k + '.npy', len(npz.npy_header(v.shape, v.dtype)) + v.nbytes) for k, v in arrays.items()]
    blob = open(ours, 'rb').read()
    assert (b'PK\x06\x06' in blob and b'PK\x06\x07' in blob) == force_zip64    # the ZIP64 end records
    if force_zip64:
        at = blob.index(b'PK\x03\x04')
        assert blob[at + 18:at + 26] == b'\xff' * 8 and blob[at + 4:at + 6] == b'\x2d\x00'   # sizes in the extra field, version 4.5


def test_write_npz_takes_empty_and_odd_members(tmp_path):
    arrays = dict(empty=np.zeros((0, 3), np.float32), scalar=np.array(7, np.int64), big=np.arange(100000, dtype=np.uint16).reshape(100, 1000))
    path = str(tmp_path / 'odd.npz')
    npz.write_npz(path, [npz.host_member(k, v) for k, v in arrays.items()])
    with np.load(path) as got:
        for k, v in arrays.items():
            assert got[k].dtype == v.dtype and got[k].shape == v.shape and np.array_equal(got[k], v)
    header = npz.npy_header((100, 1000), np.uint16)
    assert np.lib.format.read_magic(__import__('io').BytesIO(header)) == (1, 0) and len(header) % 64 == 0
    bad = npz.Member('x.npy', header, [b'\x00' * (1 << 10)], 0, 200000)
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None
    npz.write_npz(path, [bad])
    with zipfile.ZipFile(path) as z, pytest.raises(Exception):               # a producer's wrong bytes are caught by the reader
        z.read('x.npy')


# ---- who compresses ----------------------------------------------------------------------------------------------------------------
def test_compressor_rule_keyword_over_environment_over_default(monkeypatch):
    assert make_test_set.COMPRESS_ENV == 'VARSEP_NPZ_COMPRESS'
    monkeypatch.delenv(make_test_set.COMPRESS_ENV, raising=False)
    assert make_test_set.npz_compressor() == 'host' and make_test_set.npz_compressor(None) == 'host'
    monkeypatch.setenv(make_test_set.COMPRESS_ENV, '')
    assert make_test_set.npz_compressor() == 'host'                         # empty counts as unset
    for env in ('host', 'device'):
        monkeypatch.setenv(make_test_set.COMPRESS_ENV, env)
        assert make_test_set.npz_compressor() == env
        for kw in ('host', 'device'):
            assert make_test_set.npz_compressor(kw) == kw                   # the keyword over the environment
    monkeypatch.setenv(make_test_set.COMPRESS_ENV, 'gpu')
    with pytest.raises(ValueError, match=r"VARSEP_NPZ_COMPRESS='gpu'.*'host' or 'device'"):
        make_test_set.npz_compressor()
    assert make_test_set.npz_compressor('device') == 'device'
    with pytest.raises(ValueError, match=r"compress='fast'.*'host' or 'device'"):
        make_test_set.npz_compressor('fast')


def test_main_still_calls_savez_compressed_unless_told_otherwise(monkeypatch, tmp_path):
    arrays = _case_arrays()
    calls = []
    monkeypatch.setattr(make_test_set, 'generate', lambda *a, **kw: calls.append('generate') or arrays)
    monkeypatch.setattr(make_test_set, 'generate_device', lambda *a, **kw: calls.append('generate_device') or
                        {k: torch.from_numpy(v) for k, v in arrays.items()})
    monkeypatch.setattr(np, 'savez_compressed', lambda path, **kw: calls.append(('savez_compressed', path, list(kw), all(kw[k] is arrays[k] for k in kw))))
    monkeypatch.setattr(npz, 'write_npz', lambda path, members, force_zip64=False: calls.append(('write_npz', path, [m.name for m in members])))
    path = os.path.join(str(tmp_path), 'mmnist_test_2digits_64.npz')
    argv = ['--data_dir', str(tmp_path), '--device', '0']
    monkeypatch.delenv(make_test_set.COMPRESS_ENV, raising=False)
    make_test_set.main(argv)
    assert calls == ['generate', ('savez_compressed', path, list(arrays), True)]
    del calls[:]
    monkeypatch.setenv(make_test_set.COMPRESS_ENV, 'host')
    make_test_set.main(argv)
    assert calls == ['generate', ('savez_compressed', path, list(arrays), True)]
    del calls[:]
    monkeypatch.setenv(make_test_set.COMPRESS_ENV, 'zip')
    with pytest.raises(ValueError, match='VARSEP_NPZ_COMPRESS'):
        make_test_set.main(argv)
    assert calls == []                                                      # refused before anything is generated
    monkeypatch.setenv(make_test_set.COMPRESS_ENV, 'device')
    with pytest.raises(_lib.VarsepHipError):                                # the device route takes device tensors: no CPU fallback
        make_test_set.main(argv)
    assert calls == ['generate_device']
    # save_test_set's host route downloads tensors and writes the same file
    del calls[:]
    make_test_set.save_test_set(path, {k: torch.from_numpy(v) for k, v in arrays.items()}, compress='host')
    assert calls[0][:3] == ('savez_compressed', path, list(arrays))

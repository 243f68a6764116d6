"""Reading .npz members on the device, the part that needs no GPU: the declarations and argument checks of the entry points of
csrc/vs_inflate_chunks.hip, the segment decoder (csrc/vs_inflate_chunks_core.h) compiled for the host and run -- scan, segments, chain,
place, resolve -- on the corpus of tests/inflate_chunks_inputs.py against zlib, on speculative starts, truncations and corruptions; the zip
directory reader of utils/npz.py against `zipfile`; the rule that selects the reader; and that nothing changes while the rule says `host`."""
import ctypes
import os
import re
import zipfile
import zlib

import numpy as np
import pytest
import torch

import deflate_inputs as D
import inflate_chunks_inputs as IC
from spatiotemporal_variable_separation_amd import _lib, ops
from spatiotemporal_variable_separation_amd.data import moving_mnist
from spatiotemporal_variable_separation_amd.test.mnist import test_disentanglement as swap
from spatiotemporal_variable_separation_amd.test.mnist import test_disentanglement_stochastic as swap_stochastic
from spatiotemporal_variable_separation_amd.utils import loadz, npz

ENTRIES = ('vs_inflate_sync_scan', 'vs_inflate_segments', 'vs_inflate_place', 'vs_inflate_resolve', 'vs_u8_tn_to_f32_nt')
S = ops.INFLATE_SLOT_BYTES


# ---- the entry points --------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_built():
    header = open(os.path.join(D.ROOT, 'include', 'varsep_hip.h')).read()
    lib = _lib.load_library()
    for entry in ENTRIES:
        assert re.search(r'\bint %s\(' % entry, header) and entry in _lib.SIGNATURES and hasattr(lib, entry), entry
        declared = re.search(r'\bint %s\(([^;]*)\);' % entry, header).group(1)
        assert len(declared.split(',')) == len(_lib.SIGNATURES[entry][1]), entry
    assert 'vs_inflate_chunks.hip' in _lib.SOURCES and os.path.exists(os.path.join(os.path.dirname(_lib.__file__), 'csrc', 'vs_inflate_chunks.hip'))
    for macro, value in (('VS_INFLATE_SLOT_BYTES', S), ('VS_INFLATE_REPORT_WORDS', ops.INFLATE_REPORT_WORDS)):
        assert re.search(r'#define %s %d\b' % (macro, value), header), macro
    assert re.search(r'#define VS_INFLATE_MAX_BATCH %dll\b' % ops.INFLATE_MAX_BATCH, header)
    assert S == ops.DEFLATE_CHUNK == 32768 and len(IC.WORDS) == ops.INFLATE_REPORT_WORDS


def test_entry_points_refuse_null_pointers_negative_sizes_large_batches_and_short_slots():
    lib = _lib.load_library()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 1)
    big = ops.INFLATE_MAX_BATCH + 1

    def scan(comp=p, n=16, cand=p, cap=4, count=p):
        return lib.vs_inflate_sync_scan(comp, n, cand, cap, count, None)

    def segments(comp=p, n=16, cand=p, n_cand=1, slots=p, stride=S, marks=p, words=p):
        return lib.vs_inflate_segments(comp, n, cand, n_cand, slots, stride, marks, words, None)

    def place(slots=p, stride=S, n_slots=1, index=p, sizes=p, offsets=p, n=1, out=p, out_bytes=8):
        return lib.vs_inflate_place(slots, stride, n_slots, index, sizes, offsets, n, out, out_bytes, None)

    def resolve(marks=p, n_slots=1, index=p, sizes=p, offsets=p, n=1, out=p, out_bytes=8):
        return lib.vs_inflate_resolve(marks, n_slots, index, sizes, offsets, n, out, out_bytes, None)

    def convert(src=p, T=1, N=1, inner=4, dst=p):
        return lib.vs_u8_tn_to_f32_nt(src, T, N, inner, dst, None)

    refused = [
        (scan, [dict(comp=None), dict(count=None), dict(cand=None), dict(n=-1), dict(cap=-1), dict(n=(1 << 31) * 4096)]),
        (segments, [dict(comp=None), dict(cand=None), dict(slots=None), dict(marks=None), dict(words=None), dict(n=-1), dict(n_cand=-1),
                    dict(n_cand=big), dict(stride=S - 1), dict(stride=0), dict(marks=odd)]),
        (place, [dict(slots=None), dict(index=None), dict(sizes=None), dict(offsets=None), dict(out=None), dict(n=-1), dict(n_slots=-1),
                 dict(out_bytes=-1), dict(n=big), dict(n_slots=big), dict(stride=S - 1)]),
        (resolve, [dict(marks=None), dict(index=None), dict(sizes=None), dict(offsets=None), dict(out=None), dict(n=-1), dict(n_slots=-1),
                   dict(out_bytes=-1), dict(n=big), dict(n_slots=big), dict(marks=odd)]),
        (convert, [dict(src=None), dict(dst=None), dict(T=-1), dict(N=-1), dict(inner=-1), dict(T=1 << 20, N=1 << 20), dict(dst=ctypes.c_void_p(p.value + 8))]),
    ]
    for entry, (call, cases) in zip(ENTRIES, refused):
        for kwargs in cases:
            assert call(**kwargs) == -1, (entry, kwargs)
            assert lib.vs_last_error().decode().startswith(entry + ':'), (entry, kwargs)
    # nothing to do, nothing launched
    assert segments(n_cand=0) == 0 and place(n=0) == 0 and resolve(n=0) == 0 and convert(T=0) == 0 and convert(inner=0) == 0


def test_ops_refuse_host_tensors_and_bad_arguments():
    with pytest.raises(_lib.VarsepHipError):
        ops.inflate_raw(torch.zeros(10, dtype=torch.uint8), 10)
    with pytest.raises(_lib.VarsepHipError):
        ops.inflate_sync_scan(torch.zeros(10, dtype=torch.uint8))
    with pytest.raises(_lib.VarsepHipError):
        ops.u8_tn_to_f32_nt(torch.zeros(2, 2, dtype=torch.uint8))
    assert 'InflateNotChunked' in repr(ops.InflateNotChunked('why')) and ops.InflateNotChunked('why').reason == 'why'


# ---- the logic on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('inflate_chunks_host')
    corpus = IC.corpus(tmp)
    exe, sanitized = IC.compile_host_check(tmp)
    records, stdout = IC.run_host_check(exe, [(c['comp'], c['want']) for c in corpus], tmp)
    print('sanitizers:', sanitized, '|', stdout.strip().splitlines()[-1])
    assert stdout.strip().splitlines()[-1].endswith('mismatches 0'), stdout[-3000:]
    return dict(tmp=tmp, exe=exe, sanitized=sanitized, cases={c['name']: (c, r) for c, r in zip(corpus, records)})


def test_the_corpus_is_what_it_claims_to_be(host):
    cases = host['cases']
    assert len(cases) >= 300 and sum(1 for n in cases if 'mixture' in n) >= IC.N_MIXTURES
    for name, (c, _) in cases.items():
        d = zlib.decompressobj(-15)
        assert d.decompress(c['comp']) == c['want'] and d.eof and not d.unused_data, name
    assert 'runs_32768_3L_plus_5' in cases and len(cases['runs_32768_3L_plus_5'][0]['want']) == 128 + 3 * IC.L + 5
    assert IC.MARKER not in cases['foreign_10k'][0]['comp']


def test_every_chain_rebuilds_zlibs_bytes_and_no_device_written_member_falls_back(host):
    fallbacks = []
    for name, (c, r) in host['cases'].items():
        assert r['chain_ok'] == c['chains'], name
        if r['chain_ok']:
            assert r['out'] == c['want'], name
            w = r['words'][r['chain']]
            assert (w[:, 0] == 0).all() and w[-1, 2] == 1 and w[-1, 1] == len(c['comp']) and (w[:-1, 2] == 0).all(), name
            assert w[:, 3].sum() == len(c['want']) and (w[:, 3] <= S).all(), name
            assert (r['cand'][r['chain'][1:]] == w[:-1, 1]).all(), name        # every segment starts where the one before it ended
        elif c['device']:
            fallbacks.append(name)
    assert fallbacks == []                                                   # the allowed share of fallbacks is zero
    c, r = host['cases']['foreign_200k']
    assert r['words'][0, 0] == 8 and not r['chain_ok']                      # one stream without markers: VS_INFLATE_OUT_LONG, the host route
    c, r = host['cases']['foreign_10k']
    assert len(r['cand']) == 1 and len(r['chain']) == 1                     # a small foreign member is a one-segment chain
    c, r = host['cases']['runs_32768_empty']
    assert len(r['chain']) == 2 and r['words'][1, 3] == 0                   # the header piece, then the final block alone


@pytest.mark.parametrize('name', ['window_1024_video_major', 'window_1024_slab_border', 'window_32768_video_major'])
def test_the_window_cases_really_contain_external_bytes_in_chains_through_the_chunks(host, name):
    c, r = host['cases'][name]
    w = r['words'][r['chain']]
    with_ext = int((w[:, 4] > 0).sum())
    print(name, 'segments', len(w), 'with externals', with_ext, 'external bytes', int(w[:, 4].sum()), 'largest reach', int(w[:, 5].max()))
    assert w[:, 4].sum() > len(c['want']) // 4 and w[:, 5].max() > 4096
    if '1024' in name:
        assert with_ext > len(w) // 2 and w[:, 5].max() > 16 * 1024           # references many chunks back
        produced_before = np.cumsum(w[:, 3]) - w[:, 3]
        assert (w[:, 5] <= produced_before).all()


@pytest.mark.parametrize('name', ['planted_1024', 'planted_32768'])
def test_the_planted_cases_really_contain_off_chain_candidates(host, name):
    c, r = host['cases'][name]
    off_chain = len(r['cand']) - len(r['chain'])
    print(name, 'candidates', len(r['cand']), 'on the chain', len(r['chain']))
    assert off_chain == IC.PLANTED and r['chain_ok']
    assert c['comp'].count(IC.MARKER) == len(r['cand']) - 1


def test_speculative_starts_truncations_and_corruptions_end_with_a_status(host):
    names = ['runs_1024_odd_len_off3', 'foreign_10k', 'runs_1024_run_edges']
    cases = [(host['cases'][n][0]['comp'], host['cases'][n][0]['want']) for n in names]
    # a window stream small enough to be cut at every byte: its own segments, externals included
    c = host['cases']['window_1024_video_major'][0]
    r = host['cases']['window_1024_video_major'][1]
    k = 40
    cut = int(r['cand'][r['chain'][k]])
    small = c['comp'][:cut] + npz.FINAL_BLOCK
    cases.append((small, zlib.decompressobj(-15).decompress(small)))
    records, stdout = IC.run_host_check(host['exe'], cases, host['tmp'], tag='ic_damage', mode=[1] * len(cases))
    last = stdout.strip().splitlines()[-1]
    print(last)
    assert last.endswith('mismatches 0'), stdout[-3000:]
    decodes = int(re.search(r'decodes (\d+)', last).group(1))
    assert decodes > sum(len(comp) for comp, _ in cases) + 200 * len(cases)
    assert all(rec['chain_ok'] for rec in records) and records[-1]['words'][:, 4].sum() > 0


# ---- the directory reader ----------------------------------------------------------------------------------------------------------
def _check_directory(path):
    entries = npz.read_directory(path)
    raw = open(path, 'rb').read()
    with zipfile.ZipFile(path) as z:
        infos = z.infolist()
        assert len(entries) == len(infos)
        for e, i in zip(entries, infos):
            assert (e.name, e.method, e.crc32, e.csize, e.usize) == (i.filename, i.compress_type, i.CRC, i.compress_size, i.file_size)
            body = raw[e.data_offset:e.data_offset + e.csize]
            data = body if e.method == 0 else zlib.decompress(body, -15)
            assert data == z.read(i)
            h = npz.parse_npy_header(data[:4096])
            a = np.load(path, allow_pickle=True)[e.name[:-4]]
            assert h.shape == a.shape and h.dtype == a.dtype and h.header_bytes + a.nbytes == e.usize and h.fortran_order == (a.flags.f_contiguous and not a.flags.c_contiguous)
    return entries


def test_directory_reader_agrees_with_zipfile(tmp_path):
    arrays = dict(a=np.arange(5000, dtype=np.int32), b=np.zeros((3, 4), np.float32), c=np.array(7.5), d=np.zeros((0, 3), np.uint8),
                  f=np.asfortranarray(np.arange(12.).reshape(3, 4)))
    np.savez_compressed(tmp_path / 'foreign.npz', **arrays)
    np.savez(tmp_path / 'stored.npz', **arrays)
    for zip64 in (False, True):
        npz.write_npz(str(tmp_path / ('ours%d.npz' % zip64)), [npz.host_member(k, v, piece_bytes=4096) for k, v in arrays.items() if k != 'f'],
                      force_zip64=zip64)
    assert [e.method for e in _check_directory(tmp_path / 'foreign.npz')] == [8] * 5
    assert [e.method for e in _check_directory(tmp_path / 'stored.npz')] == [0] * 5
    plain, wide = _check_directory(tmp_path / 'ours0.npz'), _check_directory(tmp_path / 'ours1.npz')
    assert [e.data_offset - p.data_offset for e, p in zip(wide, plain)] == [20 * (k + 1) for k in range(4)]   # the ZIP64 extra fields
    two = io_header_2_0()
    assert npz.parse_npy_header(two).header_bytes == len(two)
    with pytest.raises(zipfile.BadZipFile):
        (tmp_path / 'not.npz').write_bytes(b'no zip file at all' * 10)
        npz.read_directory(tmp_path / 'not.npz')


def io_header_2_0():
    import io
    f = io.BytesIO()
    np.lib.format.write_array_header_2_0(f, {'descr': '<f8', 'fortran_order': False, 'shape': (3,)})
    return f.getvalue()


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def test_loader_rule_keyword_over_environment_over_default(monkeypatch):
    assert loadz.LOAD_ENV == 'VARSEP_NPZ_LOAD'
    monkeypatch.delenv(loadz.LOAD_ENV, raising=False)
    assert loadz.npz_loader() == 'host' and loadz.npz_loader(None) == 'host'
    monkeypatch.setenv(loadz.LOAD_ENV, '')
    assert loadz.npz_loader() == 'host'                                     # empty counts as unset
    for env in ('host', 'device'):
        monkeypatch.setenv(loadz.LOAD_ENV, env)
        assert loadz.npz_loader() == env
        for kw in ('host', 'device'):
            assert loadz.npz_loader(kw) == kw                               # the keyword over the environment
    monkeypatch.setenv(loadz.LOAD_ENV, 'gpu')
    with pytest.raises(ValueError, match=r"VARSEP_NPZ_LOAD='gpu'.*'host' or 'device'"):
        loadz.npz_loader()
    assert loadz.npz_loader('device') == 'device'
    with pytest.raises(ValueError, match=r"load='zlib'.*'host' or 'device'"):
        loadz.npz_loader('zlib')


def test_host_route_of_load_is_np_load_and_an_upload(tmp_path, monkeypatch):
    arrays = dict(a=np.arange(50, dtype=np.int64).reshape(5, 10), b=np.array(True), c=np.arange(3, dtype='>i4'), o=np.array([{'k': 1}], dtype=object))
    np.savez_compressed(tmp_path / 'x.npz', **arrays)
    monkeypatch.setattr(ops, 'inflate_raw', lambda *a, **k: pytest.fail('the host route decodes nothing on the device'))
    report = {}
    got = loadz.load(str(tmp_path / 'x.npz'), 'cpu', load='host', report=report)
    assert list(got) == list(arrays) and all(report[k] == ('host', 'load=host') for k in arrays)
    assert torch.equal(got['a'], torch.from_numpy(arrays['a'])) and got['b'].dtype == torch.bool and got['b'].shape == ()
    assert got['c'].dtype == torch.int32 and got['c'].tolist() == [0, 1, 2]
    assert isinstance(got['o'], np.ndarray) and got['o'][0] == {'k': 1}     # what torch cannot hold stays the host array
    assert list(loadz.load(str(tmp_path / 'x.npz'), 'cpu', keys=('b',), load='host')) == ['b']
    monkeypatch.setenv(loadz.LOAD_ENV, 'neither')
    with pytest.raises(ValueError, match='VARSEP_NPZ_LOAD'):
        loadz.load(str(tmp_path / 'x.npz'), 'cpu')


# ---- nothing changes while nothing is set --------------------------------------------------------------------------------------------
def _test_set_file(directory, prefix=''):
    rs = np.random.RandomState(3)
    sequences = rs.randint(0, 256, size=(6, 5, 1, 64, 64)).astype(np.uint8)
    latents = rs.randint(0, 36, size=(6, 5, 2, 4)).astype(np.int64)
    np.savez_compressed(os.path.join(directory, '%smmnist_test_2digits_64.npz' % prefix), sequences=sequences, latents=latents)
    return sequences, latents


@pytest.mark.parametrize('env', [None, '', 'host'])
def test_make_dataset_and_the_swap_datasets_still_call_np_load_when_nothing_is_set(tmp_path, monkeypatch, env):
    if env is None:
        monkeypatch.delenv(loadz.LOAD_ENV, raising=False)
    else:
        monkeypatch.setenv(loadz.LOAD_ENV, env)
    calls, real = [], np.load

    def spy(path, *args, **kwargs):
        calls.append((os.path.basename(str(path)), kwargs))
        return real(path, *args, **kwargs)

    monkeypatch.setattr(np, 'load', spy)
    monkeypatch.setattr(loadz, 'load', lambda *a, **k: pytest.fail('the device reader is opt-in'))
    monkeypatch.setattr(swap, 'read_mnist_images', lambda *a, **k: np.zeros((4, 28, 28), np.uint8))
    monkeypatch.setattr(swap_stochastic, 'read_mnist_images', lambda *a, **k: np.zeros((4, 28, 28), np.uint8))
    for prefix, deterministic in (('', True), ('s', False)):
        sequences, latents = _test_set_file(str(tmp_path), prefix)
        del calls[:]
        ds = moving_mnist.MovingMNIST.make_dataset(str(tmp_path), 64, 2, 6, 4, deterministic, 2, False, device='cpu')
        assert calls == [('%smmnist_test_2digits_64.npz' % prefix, {'allow_pickle': True})]
        assert ds.data.dtype == torch.float32 and torch.equal(ds.data, torch.from_numpy(sequences.swapaxes(0, 1).astype(np.float32)))
        del calls[:]
        cls = swap.SwapDataset if deterministic else swap_stochastic.StochasticSwapDataset
        sd = cls(str(tmp_path), 6, 2, 2, device='cpu')
        assert calls == [('%smmnist_test_2digits_64.npz' % prefix, {'allow_pickle': True})]
        assert sd.positions.dtype == torch.int32 and torch.equal(sd.positions, torch.from_numpy(latents[..., :2].astype(np.int32)))
        with pytest.raises(ValueError, match='latents'):
            cls(str(tmp_path), 7, 2, 2, device='cpu')


def test_the_rule_reaches_make_dataset_and_load_dataset(tmp_path, monkeypatch):
    """With `device` the file goes through loadz.load (a stand-in here: the decode itself is tests/test_npz_load_gpu.py's).  The content-swap
    scripts' own `latents` read stays np.load: their test videos come through `load_dataset`, which follows the rule."""
    from spatiotemporal_variable_separation_amd.test.mnist import test as mnist_test
    sequences, latents = _test_set_file(str(tmp_path))
    asked = []

    def stand_in(path, device, keys=None, load=None, report=None):
        asked.append((os.path.basename(path), tuple(keys), load))
        with np.load(path) as z:
            return {k: torch.from_numpy(z[k]) for k in keys}

    monkeypatch.setattr(loadz, 'load', stand_in)
    monkeypatch.setattr(ops, 'u8_tn_to_f32_nt', lambda x: x.transpose(0, 1).to(torch.float32).contiguous())
    monkeypatch.setattr(swap, 'read_mnist_images', lambda *a, **k: np.zeros((4, 28, 28), np.uint8))
    monkeypatch.setenv(loadz.LOAD_ENV, 'device')
    want = torch.from_numpy(sequences.swapaxes(0, 1).astype(np.float32))
    ds = moving_mnist.MovingMNIST.make_dataset(str(tmp_path), 64, 2, 6, 4, True, 2, False, device='cpu')
    assert asked == [('mmnist_test_2digits_64.npz', ('sequences',), 'device')] and torch.equal(ds.data, want)
    del asked[:]
    args = type('Args', (), dict(data_dir=str(tmp_path), nt_cond=2, nt_pred=4, n_object=2))()
    assert torch.equal(mnist_test.load_dataset(args, train=False, device='cpu').data, want)                 # what the content-swap scripts call
    assert torch.equal(mnist_test.load_dataset(args, train=False, device='cpu', load='device').data, want)  # what test.py's main calls
    assert asked == [('mmnist_test_2digits_64.npz', ('sequences',), 'device')] * 2
    del asked[:]
    sd = swap.SwapDataset(str(tmp_path), 6, 2, 2, device='cpu')
    assert torch.equal(sd.positions, torch.from_numpy(latents[..., :2].astype(np.int32)))
    moving_mnist.MovingMNIST.make_dataset(str(tmp_path), 64, 2, 6, 4, True, 2, False, device='cpu', load='host')   # the keyword over the environment
    mnist_test.load_dataset(args, train=False, device='cpu', load='host')
    assert asked == []
    monkeypatch.setenv(loadz.LOAD_ENV, 'gpu')
    with pytest.raises(ValueError, match='VARSEP_NPZ_LOAD'):
        moving_mnist.MovingMNIST.make_dataset(str(tmp_path), 64, 2, 6, 4, True, 2, False, device='cpu')

"""GPU: the block-parallel inflater (csrc/vs_inflate_blocks.hip) against the host build of the same logic on the corpus of
tests/inflate_blocks_inputs.py -- candidates, every report word of both decodes, the windows and the output bytes, in one batch and in
batches of 4 candidates, with guard bytes round every buffer --, utils/loadz.load with foreign='device' against np.load on NumPy-written
files, a damaged foreign member, and `MovingMNIST.make_dataset(train=False)` on a NumPy-written test file with both rules set."""
import zipfile
import zlib

import numpy as np
import pytest
import torch

import inflate_blocks_inputs as IB
from guard_util import CANARY, guarded_ops
from spatiotemporal_variable_separation_amd import _lib, ops
from spatiotemporal_variable_separation_amd.data import moving_mnist
from spatiotemporal_variable_separation_amd.utils import loadz, npz

pytestmark = pytest.mark.gpu

W, RW, DW = ops.INFLATE_WINDOW_BYTES, ops.INFLATE_REPORT_WORDS, ops.INFLATE_DECODE_WORDS
NAMES = [c['name'] for c in IB.corpus()]


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """{name: (case, record of the host build)}: the model, computed once."""
    tmp = tmp_path_factory.mktemp('inflate_blocks_gpu')
    corpus = IB.corpus()
    exe, _ = IB.compile_host_check(tmp)
    records, stdout = IB.run_host_check(exe, [(c['comp'], c['want']) for c in corpus], tmp)
    assert stdout.strip().splitlines()[-1].endswith('mismatches 0'), stdout[-3000:]
    return {c['name']: (c, r) for c, r in zip(corpus, records)}


def _dev(b):
    return torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).cuda()


def _run(monkeypatch, c, r, batch):
    """ops.inflate_blocks on one case under guard bytes: candidates, words of both decodes, windows and bytes equal the host build's."""
    comp = _dev(c['comp'])
    trace = []
    with monkeypatch.context() as m:
        allocs = guarded_ops(m)
        cand = ops.inflate_block_scan(comp)
        got = ops.inflate_blocks(comp, len(c['want']), crc=zlib.crc32(c['want']), batch=batch, trace=trace)
        torch.cuda.synchronize()
        allocs.check()
    name = c['name']
    assert np.array_equal(cand.cpu().numpy(), r['cand']), name
    seen, chain = np.zeros(len(r['cand']), bool), []
    for t in trace:
        if 'first' not in t:
            continue
        lo, w = t['first'], t['words']
        assert w.shape[1] == RW and np.array_equal(w, r['words'][lo:lo + len(w)]), (name, lo)
        seen[lo:lo + len(w)] = True
        if t['windows'] is None:
            assert t['chain'] == [] and t['words2'] is None
            continue
        k0 = len(chain)
        chain += [lo + row for row in t['chain']]
        assert t['words2'].shape == (len(t['chain']), DW) and np.array_equal(t['words2'], r['words2'][k0:len(chain)]), (name, lo)
        assert t['windows'].shape == (len(t['chain']) + 1, W)
        for k in range(len(t['chain']) + 1):                                 # row 0: the window handed over from the batch before
            assert zlib.crc32(t['windows'][k].tobytes()) == r['window_crc'][k0 + k], (name, lo, k)
    if r['chain_ok']:
        assert chain == r['chain'].tolist() and seen[r['chain']].all(), name
        assert trace[-1]['candidates'] == len(r['cand']) and trace[-1]['chain'] == len(chain), name
        assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and got.is_cuda and got.cpu().numpy().tobytes() == c['want'], name
    else:
        assert isinstance(got, ops.InflateNotChunked) and got.reason, name
    return seen, got


@pytest.mark.parametrize('batch', [ops.INFLATE_BATCH, 4])
@pytest.mark.parametrize('name', NAMES)
def test_kernels_equal_the_host_build(host, monkeypatch, name, batch):
    c, r = host[name]
    assert r['chain_ok'] == c['chains']
    seen, got = _run(monkeypatch, c, r, batch)
    if batch == ops.INFLATE_BATCH:
        assert seen.all()                                                   # one batch: every candidate is probed, the false ones included
    if name == 'fixed_above_cap':
        assert 'more than %d bytes of input' % ops.INFLATE_BLOCKS_MAX_IN in got.reason and r['words'][0, 0] == ops.INFLATE_CAP
    if name == 'planted_headers':
        assert len(r['cand']) - len(r['chain']) >= 100


@pytest.mark.parametrize('name', ['planted_headers', 'fixed_above_cap', 'video_major_mem1', 'text_small_mem1'])
def test_probe_windows_and_decode_write_only_what_is_theirs(host, name):
    """The entry points themselves with 0xFF everywhere: rows before and behind, the cells behind a span's tail, the bytes round `out`."""
    lib = _lib.load_library()
    c, r = host[name]
    comp, n_cand = _dev(c['comp']), len(r['cand'])
    cand = torch.from_numpy(r['cand'].copy()).cuda()
    cells = torch.full((n_cand + 2, W), -1, dtype=torch.int16, device='cuda')
    words = torch.full((n_cand + 2, RW), -1, dtype=torch.int64, device='cuda')
    _lib.check(lib.vs_inflate_block_probe(comp.data_ptr(), comp.numel(), cand.data_ptr(), n_cand, 0, n_cand, cells[1:].data_ptr(), words[1:].data_ptr(),
                                          _lib.stream_ptr()), 'probe')
    torch.cuda.synchronize()
    assert (cells[0] == -1).all() and (cells[-1] == -1).all() and (words[0] == -1).all() and (words[-1] == -1).all()
    w = words[1:-1].cpu().numpy()
    assert np.array_equal(w, r['words'])
    cells_h = cells[1:-1].cpu().numpy()
    for k in range(n_cand):
        kept = min(int(w[k, 3]), W)
        assert (cells_h[k, kept:] == -1).all(), k                            # nothing behind the tail
        if w[k, 0] == 0:
            marks = cells_h[k, :kept].astype(np.uint16)
            assert ((marks & 0x8000) == 0).all() or w[k, 4] > 0, k
            assert ((marks & 0x7F00) == 0)[(marks & 0x8000) == 0].all(), k    # a value is a byte
    if not r['chain_ok']:
        return
    chain = r['chain']
    sizes = w[chain, 3]
    offsets = np.cumsum(sizes) - sizes
    table = torch.from_numpy(np.stack([chain, r['cand'][chain], w[chain, 1], offsets, sizes]).astype(np.int64)).cuda()
    n = len(chain)
    windows = torch.full((n + 3, W), CANARY, dtype=torch.uint8, device='cuda')
    windows[1].zero_()
    _lib.check(lib.vs_inflate_block_windows(cells[1:].data_ptr(), n_cand, table[0].data_ptr(), table[4].data_ptr(), n, windows[1:].data_ptr(),
                                            _lib.stream_ptr()), 'windows')
    torch.cuda.synchronize()
    assert (windows[0] == CANARY).all() and (windows[-1] == CANARY).all()
    win_h = windows[1:-1].cpu().numpy()
    assert [zlib.crc32(row.tobytes()) for row in win_h] == r['window_crc'].tolist()
    n_out, pad = len(c['want']), 4096
    out = torch.full((n_out + 2 * pad,), CANARY, dtype=torch.uint8, device='cuda')
    mid = out[pad:pad + n_out]
    words2 = torch.full((n + 2, DW), -1, dtype=torch.int64, device='cuda')
    _lib.check(lib.vs_inflate_block_decode(comp.data_ptr(), comp.numel(), table[1].data_ptr(), table[2].data_ptr(), table[3].data_ptr(), table[4].data_ptr(),
                                           n, windows[1:].data_ptr(), mid.data_ptr(), n_out, words2[1:].data_ptr(), _lib.stream_ptr()), 'decode')
    torch.cuda.synchronize()
    assert mid.cpu().numpy().tobytes() == c['want']
    assert (out[:pad] == CANARY).all() and (out[pad + n_out:] == CANARY).all()
    assert (words2[0] == -1).all() and (words2[-1] == -1).all() and np.array_equal(words2[1:-1].cpu().numpy(), r['words2'])
    # spans whose bytes would leave the output write nothing and say so; a slot that does not exist passes its window on
    before = out.clone()
    bad = torch.tensor([[0, 0, 0], [0, 0, 0], [1 << 40, 1 << 40, 1 << 40], [n_out, -1, 0], [1, 5, -1]], dtype=torch.int64, device='cuda')
    _lib.check(lib.vs_inflate_block_decode(comp.data_ptr(), comp.numel(), bad[1].data_ptr(), bad[2].data_ptr(), bad[3].data_ptr(), bad[4].data_ptr(), 3,
                                           windows[1:].data_ptr(), mid.data_ptr(), n_out, words2[1:].data_ptr(), _lib.stream_ptr()), 'decode')
    torch.cuda.synchronize()
    assert torch.equal(out, before) and (words2[1:4, 0] == 8).all() and (words2[1:4, 2] == 0).all()
    keep = windows[1:4].clone()
    gone = torch.tensor([[n_cand, -1], [5, 5]], dtype=torch.int64, device='cuda')
    _lib.check(lib.vs_inflate_block_windows(cells[1:].data_ptr(), n_cand, gone[0].data_ptr(), gone[1].data_ptr(), 2, windows[1:].data_ptr(),
                                            _lib.stream_ptr()), 'windows')
    torch.cuda.synchronize()
    assert torch.equal(windows[2], keep[0]) and torch.equal(windows[3], keep[0]) and (windows[0] == CANARY).all()


# ---- utils/loadz.load --------------------------------------------------------------------------------------------------------------
def _arrays():
    rs = np.random.RandomState(11)
    frames = np.zeros((5, 6, 1, 64, 64), np.uint8)                          # video-major: the previous frame 4096 bytes back
    frames[:, :, 0, 20:40, 10:30] = rs.randint(0, 256, size=(5, 1, 20, 20))
    return dict(u8=frames, i32=rs.randint(-5, 5, size=(300, 70)).astype(np.int32), i64=np.arange(20000, dtype=np.int64).reshape(100, 200),
                f32=rs.rand(4000).astype(np.float32), f64=np.linspace(0, 1, 9000), flag=rs.rand(50000) < 0.1, noise=rs.randint(0, 256, 70000).astype(np.uint8),
                scalar=np.array(3, np.int32), none=np.zeros((0, 4), np.float32), one=np.array([200], np.uint8),
                text=np.frombuffer(IB.text(200000, seed=15), np.uint8))


def _same(got, want):
    for k, a in want.items():
        t = got[k]
        assert isinstance(t, torch.Tensor) and t.is_cuda and tuple(t.shape) == a.shape, k
        h = t.cpu().numpy()
        assert h.dtype == a.dtype and h.tobytes() == np.ascontiguousarray(a).tobytes(), k


def test_load_with_foreign_device_reads_numpy_written_members_on_the_device(tmp_path, monkeypatch):
    arrays = _arrays()
    extra = dict(fortran=np.asfortranarray(np.arange(12.).reshape(3, 4)), be=np.arange(5, dtype='>i4'),
                 rec=np.zeros(3, dtype=[('a', '<i4'), ('b', '<f4')]), obj=np.array([{'k': 1}, None], dtype=object))
    path = str(tmp_path / 'foreign.npz')
    np.savez_compressed(path, **arrays, **extra)
    monkeypatch.delenv(loadz.FOREIGN_ENV, raising=False)
    report = {}
    got = loadz.load(path, 'cuda', load='device', foreign='device', report=report)
    with np.load(path, allow_pickle=True) as z:
        _same(got, {k: z[k] for k in arrays})
    _same(got, dict(arrays, fortran=extra['fortran']))
    assert {k: report[k][0] for k in arrays} == {k: 'device' for k in arrays}, report
    assert report['text'] == report['u8'] == report['noise'] == ('device', 'chained at its block headers')
    assert report['fortran'] == ('host', 'Fortran order') and report['be'] == ('host', 'big-endian')
    assert report['rec'] == ('host', 'structured dtype') and report['obj'] == ('host', 'object array')
    assert got['be'].tolist() == [0, 1, 2, 3, 4] and isinstance(got['rec'], np.ndarray) and got['obj'][0] == {'k': 1}
    calls, real = [], np.load
    with monkeypatch.context() as m:                                        # np.load is not called for the covered members
        m.setattr(np, 'load', lambda p, *a, **k: (calls.append(str(p)), real(p, *a, **k))[1])
        m.setenv(loadz.FOREIGN_ENV, 'device')
        _same(loadz.load(path, 'cuda', keys=tuple(arrays), load='device'), arrays)
        assert calls == []
        # the same call with foreign='host': the same arrays with the routes of before
        report = {}
        _same(loadz.load(path, 'cuda', keys=tuple(arrays), load='device', foreign='host', report=report), arrays)
        assert len(calls) == 1
    assert report['text'][0] == report['u8'][0] == report['noise'][0] == 'host' and report['text'][1].startswith('not chunked')
    assert report['scalar'][0] == report['f32'][0] == 'device' and report['f32'][1] == 'chained at its sync markers'


def _flip(path, at):
    with open(path, 'r+b') as f:
        f.seek(at)
        b = f.read(1)[0]
        f.seek(at)
        f.write(bytes([b ^ 0x10]))


def test_a_flipped_byte_in_a_foreign_member_raises_or_gives_the_right_data(tmp_path):
    a = np.frombuffer(IB.text(200000, seed=16), np.uint8)
    path = str(tmp_path / 'text.npz')
    np.savez_compressed(path, text=a)
    (e,) = npz.read_directory(path)
    report = {}
    _same(loadz.load(path, 'cuda', load='device', foreign='device', report=report), dict(text=a))
    assert report['text'][0] == 'device'
    raised = 0
    for at in (200, e.csize // 3, e.csize // 2, e.csize - 30):
        _flip(path, e.data_offset + at)
        try:
            got = loadz.load(path, 'cuda', load='device', foreign='device')
        except (zipfile.BadZipFile, zlib.error, ValueError) as exc:
            print(at, type(exc).__name__, exc)
            raised += 1
        else:
            assert np.array_equal(got['text'].cpu().numpy(), a), 'a flipped byte at %d gave wrong data without an error' % at
        _flip(path, e.data_offset + at)
    assert raised >= 3
    _same(loadz.load(path, 'cuda', load='device', foreign='device'), dict(text=a))


# ---- the Moving-MNIST test set -----------------------------------------------------------------------------------------------------
def test_make_dataset_reads_a_numpy_written_test_file_on_the_device_bit_for_bit(tmp_path, monkeypatch):
    rs = np.random.RandomState(3)
    sequences = np.zeros((6, 5, 1, 64, 64), np.uint8)
    for t in range(6):
        sequences[t, :, 0, 5 + 4 * t:33 + 4 * t, 8:36] = rs.randint(0, 256, size=(5, 28, 28)) * (rs.rand(5, 28, 28) < 0.3)
    latents = rs.randint(0, 36, size=(6, 5, 2, 4)).astype(np.int64)
    np.savez_compressed(str(tmp_path / 'mmnist_test_2digits_64.npz'), sequences=sequences, latents=latents)
    monkeypatch.delenv(loadz.LOAD_ENV, raising=False)
    monkeypatch.delenv(loadz.FOREIGN_ENV, raising=False)
    want = moving_mnist.MovingMNIST.make_dataset(str(tmp_path), 64, 2, 6, 4, True, 2, False, device='cuda')
    calls, real = [], np.load
    monkeypatch.setattr(np, 'load', lambda p, *a, **k: (calls.append(str(p)), real(p, *a, **k))[1])
    monkeypatch.setenv(loadz.LOAD_ENV, 'device')
    monkeypatch.setenv(loadz.FOREIGN_ENV, 'device')
    report = {}
    got = moving_mnist.MovingMNIST.make_dataset(str(tmp_path), 64, 2, 6, 4, True, 2, False, device='cuda', report=report)
    assert calls == [] and report['sequences'][0] == 'device' and report['sequences'] == ('device', 'chained at its block headers')
    assert got.data.dtype == want.data.dtype == torch.float32 and got.data.shape == want.data.shape == (5, 6, 1, 64, 64)
    assert got.data.is_cuda and torch.equal(got.data, want.data) and len(got) == len(want) == 5
    monkeypatch.setenv(loadz.FOREIGN_ENV, 'host')                           # the first rule alone: the host route for this file, as before
    report = {}
    again = moving_mnist.MovingMNIST.make_dataset(str(tmp_path), 64, 2, 6, 4, True, 2, False, device='cuda', report=report)
    assert len(calls) == 1 and report['sequences'][0] == 'host' and torch.equal(again.data, want.data)

"""GPU: the stored-block finder (vs_inflate_block_scan_stored in csrc/vs_inflate_blocks.hip) and the block-parallel inflater on its
candidates against the host build of the same logic (tests/host/inflate_stored_host_check.cpp) on the corpus of
tests/inflate_stored_inputs.py -- the union list, every report word of both decodes, the windows and the output bytes, in one batch and in
batches of 4 candidates, with guard bytes round every buffer --; the entry point alone on streams of a few bytes and at both ends of a
stream; and utils/loadz.load with finder='all' against np.load on a NumPy-written file whose member is above the span allowance."""
import zlib

import numpy as np
import pytest
import torch

import inflate_blocks_inputs as IB
import inflate_stored_inputs as IS
from guard_util import guarded_ops
from spatiotemporal_variable_separation_amd import _lib, ops
from spatiotemporal_variable_separation_amd.utils import loadz

pytestmark = pytest.mark.gpu

W, RW, DW = ops.INFLATE_WINDOW_BYTES, ops.INFLATE_REPORT_WORDS, ops.INFLATE_DECODE_WORDS
NAMES = [c['name'] for c in IS.corpus()]


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """{name: (case, record of the host build with both finders)}: the model, computed once."""
    tmp = tmp_path_factory.mktemp('inflate_stored_gpu')
    corpus = IS.corpus()
    exe, _ = IS.compile_host_check(tmp)
    records, stdout = IS.run_host_check(exe, [(c['comp'], c['want']) for c in corpus], tmp)
    assert stdout.strip().splitlines()[-1].endswith('mismatches 0'), stdout[-3000:]
    return {c['name']: (c, r) for c, r in zip(corpus, records)}


def _dev(b):
    return torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).cuda()


def _run(monkeypatch, c, r, batch):
    """ops.inflate_blocks(stored=True) on one case under guard bytes: candidates, words of both decodes, windows and bytes equal the host
    build's (the comparison of test_npz_blocks_gpu._run)."""
    comp = _dev(c['comp'])
    trace = []
    with monkeypatch.context() as m:
        allocs = guarded_ops(m)
        cand = ops.inflate_block_scan(comp, stored=True)
        dynamic = ops.inflate_block_scan(comp)
        got = ops.inflate_blocks(comp, len(c['want']), crc=zlib.crc32(c['want']), batch=batch, trace=trace, stored=True)
        torch.cuda.synchronize()
        allocs.check()
    name = c['name']
    assert np.array_equal(cand.cpu().numpy(), r['cand']), name
    seen, chain = np.zeros(len(r['cand']), bool), []
    for t in trace:
        if 'first' not in t:
            continue
        lo, w = t['first'], t['words']
        assert np.array_equal(t['cand'], r['cand']), name
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
    assert r['chain_ok'] and chain == r['chain'].tolist() and seen[r['chain']].all(), name
    assert trace[-1]['candidates'] == len(r['cand']) and trace[-1]['chain'] == len(chain), name
    assert trace[-1]['stored_candidates'] == len(r['cand']) - dynamic.numel(), name
    assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and got.is_cuda and got.cpu().numpy().tobytes() == c['want'], name
    return seen


@pytest.mark.parametrize('batch', [ops.INFLATE_BATCH, 4])
@pytest.mark.parametrize('name', NAMES)
def test_kernels_equal_the_host_build(host, monkeypatch, name, batch):
    c, r = host[name]
    seen = _run(monkeypatch, c, r, batch)
    if batch == ops.INFLATE_BATCH:
        assert seen.all()                                                   # one batch: every candidate is probed, the false ones included
    if name == 'planted_stored':
        assert len(r['cand']) - len(r['chain']) >= 8 * IS.PLANTED


def test_without_the_keyword_a_member_above_the_allowance_is_not_chunked(host):
    c, r = host['random_above_cap']
    comp = _dev(c['comp'])
    assert ops.inflate_block_scan(comp).tolist() == [0]
    trace = []
    got = ops.inflate_blocks(comp, len(c['want']), crc=zlib.crc32(c['want']), trace=trace)
    assert isinstance(got, ops.InflateNotChunked) and 'more than %d bytes of input' % ops.INFLATE_BLOCKS_MAX_IN in got.reason
    assert all('stored_candidates' not in t for t in trace)


# ---- the entry point alone ---------------------------------------------------------------------------------------------------------
def _scan(data, cap=None, before=0):
    """vs_inflate_block_scan_stored on `data` (placed `before` bytes into its buffer) with 0xFF round the list and round the count:
    (sorted positions, count)."""
    lib = _lib.load_library()
    want = IS.stored_candidates(data)
    cap = len(want) if cap is None else cap
    buf = torch.full((before + len(data) + 8,), 0xA5, dtype=torch.uint8, device='cuda')
    if len(data):
        buf[before:before + len(data)] = _dev(data)
    cand = torch.full((cap + 16,), -1, dtype=torch.int64, device='cuda')
    count = torch.full((3,), -1, dtype=torch.int64, device='cuda')
    count[1] = 0
    _lib.check(lib.vs_inflate_block_scan_stored(buf[before:].data_ptr(), len(data), cand[8:].data_ptr(), cap, count[1:].data_ptr(), _lib.stream_ptr()),
               'vs_inflate_block_scan_stored')
    torch.cuda.synchronize()
    found = int(count[1])
    assert count[0] == -1 and count[2] == -1 and (cand[:8] == -1).all() and (cand[8 + min(cap, found):] == -1).all()   # it writes nothing else
    assert (buf[:before] == 0xA5).all() and (buf[before + len(data):] == 0xA5).all()
    return sorted(cand[8:8 + min(cap, found)].tolist()), found


MARKER = bytes([0x00, 0x00, 0xff, 0xff])


@pytest.mark.parametrize('before', [0, 1, 3])
def test_the_entry_point_on_streams_of_a_few_bytes_and_at_both_ends(before):
    rs = np.random.RandomState(71)
    noise = rs.randint(1, 256, size=3000).astype(np.uint8).tobytes()        # no zero byte: no zero bits in front by chance
    streams = [b'', b'\x00', MARKER[:3], MARKER,                              # 0, 1, 3 and 4 bytes: nothing to find, nothing read
               MARKER + b'\x03',                                            # B = 0: every q is negative
               b'\x00' + MARKER + b'\x03',                                  # B = 1: q = 5 .. 0, k = 6 and 7 would be negative
               b'\x01' + MARKER + b'\x03', b'\x80' + MARKER + b'\x03',
               noise + b'\x00\x00' + MARKER + b'\x03',                     # a boundary in the last five bytes, the last one that can be
               noise + b'\x00\x00' + MARKER,                               # ... and in the last four: nothing behind it, no candidate
               noise[:1021] + b'\x00\x00' + b'\x02\x00\xfd\xff' + noise[:300],   # a boundary astride two threads and two workgroups
               b'\x00' * 40 + MARKER * 3 + b'\x00' * 9 + b'\x03']
    for data in streams:
        want = IS.stored_candidates(data)
        got, found = _scan(data, before=before)
        assert got == want and found == len(want), (len(data), got[:10], want[:10])
    assert IS.stored_candidates(streams[5]) == [0, 1, 2, 3, 4, 5] and IS.stored_candidates(streams[8])[-1] == 8 * 3002 - 3
    assert len(IS.stored_candidates(streams[8])) == 8 and IS.stored_candidates(streams[9]) == []


def test_the_entry_point_counts_past_the_capacity_and_counts_alone(host):
    c, r = host['planted_stored']
    want = IS.stored_candidates(c['comp'])
    assert len(want) >= 8 * IS.PLANTED
    got, found = _scan(c['comp'])
    assert got == want and found == len(want)
    got, found = _scan(c['comp'], cap=100)
    assert found == len(want) and len(got) == 100 and set(got) <= set(want)
    lib = _lib.load_library()
    comp = _dev(c['comp'])
    count = torch.zeros((1,), dtype=torch.int64, device='cuda')
    _lib.check(lib.vs_inflate_block_scan_stored(comp.data_ptr(), comp.numel(), None, 0, count.data_ptr(), _lib.stream_ptr()), 'count')
    assert int(count[0]) == len(want)


# ---- utils/loadz.load --------------------------------------------------------------------------------------------------------------
def test_load_with_finder_all_reads_an_incompressible_member_on_the_device(tmp_path, monkeypatch):
    rs = np.random.RandomState(81)
    arrays = dict(noise=rs.randint(0, 256, size=IB.MAX_IN + 70000).astype(np.uint8), small=rs.rand(20000).astype(np.float32))   # (80 KB: above what one segment of the sync-marker reader holds)
    path = str(tmp_path / 'noise.npz')
    np.savez_compressed(path, **arrays)
    monkeypatch.delenv(loadz.FOREIGN_ENV, raising=False)
    monkeypatch.delenv(loadz.FINDER_ENV, raising=False)

    def run(**kwargs):
        report = {}
        got = loadz.load(path, 'cuda', load='device', report=report, **kwargs)
        with np.load(path) as z:
            for k, a in arrays.items():
                h = got[k].cpu().numpy()
                assert got[k].is_cuda and h.dtype == a.dtype and h.shape == a.shape and h.tobytes() == z[k].tobytes() == a.tobytes(), k
        return report

    report = run(foreign='device', finder='all')
    assert report['noise'] == report['small'] == ('device', 'chained at its block headers')
    report = run(foreign='device')                                          # the default: today's route for this file
    assert report['noise'][0] == 'host' and report['noise'][1].startswith('not chunked') and 'bytes of input' in report['noise'][1]
    assert report['small'][0] == 'device'
    monkeypatch.setenv(loadz.FOREIGN_ENV, 'device')
    monkeypatch.setenv(loadz.FINDER_ENV, 'all')                             # the environment alone does what the keywords do
    report = run()
    assert report['noise'] == report['small'] == ('device', 'chained at its block headers')
    report = run(finder='dynamic')
    assert report['noise'][0] == 'host'

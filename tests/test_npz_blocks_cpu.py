"""Reading foreign .npz members on the device, the part that needs no GPU: the declarations and argument checks of the entry points of
csrc/vs_inflate_blocks.hip; the logic (csrc/vs_inflate_blocks_core.h) compiled for the host and run -- scan, probe, chain, windows, decode
-- on the corpus of tests/inflate_blocks_inputs.py against zlib, with one lane and with threads playing 3 and 64 lanes, on false candidates,
truncations and bit flips; the finder against a block walker that is not the code under test; the rule that selects the reader of a foreign
member; and that nothing changes while that rule says `host`."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest
import torch

import deflate_inputs as D
import inflate_blocks_inputs as IB
from spatiotemporal_variable_separation_amd import _lib, ops
from spatiotemporal_variable_separation_amd.data import moving_mnist
from spatiotemporal_variable_separation_amd.utils import loadz

ENTRIES = ('vs_inflate_block_scan', 'vs_inflate_block_probe', 'vs_inflate_block_windows', 'vs_inflate_block_decode')
W = ops.INFLATE_WINDOW_BYTES


# ---- the entry points --------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_built():
    header = open(os.path.join(D.ROOT, 'include', 'varsep_hip.h')).read()
    lib = _lib.load_library()
    for entry in ENTRIES:
        assert re.search(r'\bint %s\(' % entry, header) and entry in _lib.SIGNATURES and hasattr(lib, entry), entry
        declared = re.search(r'\bint %s\(([^;]*)\);' % entry, header).group(1)
        assert len(declared.split(',')) == len(_lib.SIGNATURES[entry][1]), entry
    csrc = os.path.join(os.path.dirname(_lib.__file__), 'csrc')
    assert 'vs_inflate_blocks.hip' in _lib.SOURCES and os.path.exists(os.path.join(csrc, 'vs_inflate_blocks.hip'))
    assert os.path.exists(os.path.join(csrc, 'vs_inflate_blocks_core.h'))
    for macro, value in (('VS_INFLATE_WINDOW_BYTES', W), ('VS_INFLATE_BLOCKS_MAX_IN', ops.INFLATE_BLOCKS_MAX_IN), ('VS_INFLATE_CAP', ops.INFLATE_CAP),
                         ('VS_INFLATE_DECODE_WORDS', ops.INFLATE_DECODE_WORDS)):
        assert re.search(r'#define %s %d\b' % (macro, value), header), macro
    assert W == IB.WINDOW == 32768 and ops.INFLATE_BLOCKS_MAX_IN == IB.MAX_IN == 1 << 20 and ops.INFLATE_CAP == IB.CAP_STATUS
    assert ops.INFLATE_CAP not in ops.INFLATE_STATUS and len(IB.WORDS) == ops.INFLATE_REPORT_WORDS


def test_entry_points_refuse_null_pointers_negative_sizes_large_batches_and_odd_addresses():
    lib = _lib.load_library()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    odd = ctypes.c_void_p(p.value + 1)
    big = ops.INFLATE_MAX_BATCH + 1

    def scan(comp=p, n=16, cand=p, cap=4, count=p):
        return lib.vs_inflate_block_scan(comp, n, cand, cap, count, None)

    def probe(comp=p, n=16, cand=p, n_cand=1, first=0, m=1, cells=p, words=p):
        return lib.vs_inflate_block_probe(comp, n, cand, n_cand, first, m, cells, words, None)

    def windows(cells=p, n_slots=1, index=p, produced=p, n=1, win=p):
        return lib.vs_inflate_block_windows(cells, n_slots, index, produced, n, win, None)

    def decode(comp=p, nbytes=16, starts=p, ends=p, offsets=p, sizes=p, n=1, win=p, out=p, out_bytes=8, words=p):
        return lib.vs_inflate_block_decode(comp, nbytes, starts, ends, offsets, sizes, n, win, out, out_bytes, words, None)

    refused = [
        (scan, [dict(comp=None), dict(count=None), dict(cand=None), dict(n=-1), dict(cap=-1), dict(n=(1 << 31) * 1024)]),
        (probe, [dict(comp=None), dict(cand=None), dict(cells=None), dict(words=None), dict(n=-1), dict(n_cand=-1), dict(first=-1), dict(m=-1),
                 dict(m=big, n_cand=big), dict(first=1), dict(m=2), dict(first=1, m=1, n_cand=1), dict(cells=odd)]),
        (windows, [dict(cells=None), dict(index=None), dict(produced=None), dict(win=None), dict(n=-1), dict(n_slots=-1), dict(n=big),
                   dict(n_slots=big), dict(cells=odd), dict(win=ctypes.c_void_p(p.value + 8))]),
        (decode, [dict(comp=None), dict(starts=None), dict(ends=None), dict(offsets=None), dict(sizes=None), dict(win=None), dict(out=None),
                  dict(words=None), dict(nbytes=-1), dict(n=-1), dict(out_bytes=-1), dict(n=big), dict(win=ctypes.c_void_p(p.value + 4))]),
    ]
    for entry, (call, cases) in zip(ENTRIES, refused):
        for kwargs in cases:
            assert call(**kwargs) == -1, (entry, kwargs)
            assert lib.vs_last_error().decode().startswith(entry + ':'), (entry, kwargs)
    # nothing to do, nothing launched
    assert probe(m=0) == 0 and probe(m=0, n_cand=0) == 0 and windows(n=0) == 0 and decode(n=0) == 0


def test_ops_refuse_host_tensors_and_bad_arguments():
    with pytest.raises(_lib.VarsepHipError):
        ops.inflate_blocks(torch.zeros(10, dtype=torch.uint8), 10)
    with pytest.raises(_lib.VarsepHipError):
        ops.inflate_block_scan(torch.zeros(10, dtype=torch.uint8))


# ---- the logic on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """The host build on the whole corpus with one lane (the damage runs included) and with threads playing 3 and 64 lanes."""
    tmp = tmp_path_factory.mktemp('inflate_blocks_host')
    corpus = IB.corpus()
    exe, sanitized = IB.compile_host_check(tmp)
    cases = [(c['comp'], c['want']) for c in corpus]
    runs = {}
    for lanes in (1, 3, 64):
        records, stdout = IB.run_host_check(exe, cases, tmp, tag='ib_%d' % lanes, mode=[int(c['damage']) for c in corpus] if lanes == 1 else None,
                                            lanes=lanes)
        last = stdout.strip().splitlines()[-1]
        print('sanitizers:', sanitized, '|', last)
        assert last.startswith('lanes %d ' % lanes) and last.endswith('mismatches 0'), stdout[-3000:]
        runs[lanes] = dict(records=records, last=last)
    return dict(tmp=tmp, exe=exe, sanitized=sanitized, runs=runs, cases={c['name']: (c, r) for c, r in zip(corpus, runs[1]['records'])})


def _count(blocks, btype):
    return sum(1 for b in blocks if b['type'] == btype)


def test_the_corpus_is_what_it_claims_to_be(host):
    """Per stream: zlib inflates it to its bytes, the block walker counts the blocks it claims, and the finder's candidates are bit 0, every
    non-final dynamic block start and the planted headers -- nothing is missed and nothing else is found."""
    cases = host['cases']
    assert len(cases) >= 19
    found = missed = 0
    for name, (c, r) in cases.items():
        d = zlib.decompressobj(-15)
        assert d.decompress(c['comp']) == c['want'] and d.eof and not d.unused_data, name
        blocks, claims = IB.walk_blocks(c['comp']), c['claims']
        stored, fixed, dynamic = (_count(blocks, t) for t in (0, 1, 2))
        print(name, 'bytes', len(c['want']), 'compressed', len(c['comp']), 'stored/fixed/dynamic', stored, fixed, dynamic, 'candidates', len(r['cand']))
        assert [b['end'] for b in blocks[:-1]] == [b['start'] for b in blocks[1:]] and blocks[0]['start'] == 0 and blocks[-1]['final'], name
        assert len(blocks) == claims.get('blocks', len(blocks)) and len(blocks) <= claims.get('max_blocks', len(blocks)), name
        assert dynamic >= claims.get('min_dynamic', 0) and stored >= claims.get('min_stored', 0) and fixed >= claims.get('min_fixed', 0), name
        if claims.get('only_stored'):
            assert stored == len(blocks), name
        if claims.get('only_fixed'):
            assert fixed == len(blocks), name
        assert len(c['comp']) >= claims.get('min_comp', 0), name
        truth = {0} | {b['start'] for b in blocks if b['type'] == 2 and not b['final']}
        if 'planted' in claims:
            at, spots = c['comp'].find(claims['planted']), set()
            while at >= 0:
                spots.add(8 * at)
                at = c['comp'].find(claims['planted'], at + 1)
            assert len(spots) >= 100 and not spots & truth, name
            truth |= spots
        cand = r['cand'].tolist()
        assert cand == sorted(set(cand)), name
        missed += len(truth - set(cand))
        found += len(set(cand) - truth)
        assert set(cand) == truth, (name, sorted(truth - set(cand))[:5], sorted(set(cand) - truth)[:5])
    assert (missed, found) == (0, 0)


def test_every_chain_rebuilds_zlibs_bytes_and_nothing_that_must_chain_falls_back(host):
    for name, (c, r) in host['cases'].items():
        assert r['chain_ok'] == c['chains'], (name, r['fail'])
        if not r['chain_ok']:
            continue
        assert r['out'] == c['want'], name
        w = r['words'][r['chain']]
        assert (w[:, 0] == 0).all() and w[-1, 2] == 1 and (w[-1, 1] + 7) // 8 == len(c['comp']) and (w[:-1, 2] == 0).all(), name
        assert w[:, 3].sum() == len(c['want']), name
        assert (r['cand'][r['chain'][1:]] == w[:-1, 1]).all(), name            # every span starts at the bit where the one before it ended
        assert (w[:, 5] <= np.cumsum(w[:, 3]) - w[:, 3]).all(), name           # no reach before the stream
        assert (r['words2'] == w[:, [0, 1, 3]]).all(), name                    # the second decode reports what the probe did
        assert r['window_crc'][0] == zlib.crc32(bytes(W)), name
        data = bytes(W) + c['want']                                           # the windows are the bytes before every span, zeros before the stream
        ends = np.cumsum(w[:, 3])
        for k in {0, len(w) // 2, len(w) - 1}:
            assert r['window_crc'][k + 1] == zlib.crc32(data[int(ends[k]):int(ends[k]) + W]), (name, k)
        claims = c['claims']
        assert w[:, 5].max() >= claims.get('min_reach', 0) and w[:, 3].max() >= claims.get('min_produced', 0), name
        assert w[:, 4].sum() >= claims.get('min_external_share', 0) * len(c['want']), name
        assert w[:, 3].mean() <= claims.get('max_mean_produced', 1 << 40), name
    c, r = host['cases']['fixed_above_cap']
    assert r['words'][0, 0] == IB.CAP_STATUS and r['fail'] == 1 and len(r['cand']) == 1
    assert IB.MAX_IN * 8 - 64 <= r['words'][0, 1] <= (IB.MAX_IN + 1) * 8       # the probe stopped at its allowance, not at the end of the stream
    c, r = host['cases']['planted_headers']
    assert len(r['chain']) == 1 and len(r['cand']) - 1 >= 100 and (r['words'][1:, 0] != 0).sum() >= 100   # false candidates, decoded and ignored
    c, r = host['cases']['zeros_4MiB']
    assert r['words'][r['chain'], 3].max() >= 128 * W                        # the ring wrapped many times
    c, r = host['cases']['floats_level1_mem2']
    kinds = {b['type'] for b in IB.walk_blocks(c['comp'])}
    assert kinds == {0, 1, 2} and len(r['chain']) >= 3                         # stored, fixed and dynamic blocks in one chain
    c, r = host['cases']['period_30000x20']
    assert (r['words'][r['chain'][2:], 4] > 0).all()                          # a byte's source chain runs through every span


def test_threads_playing_3_and_64_lanes_give_the_one_lane_records(host):
    one = host['runs'][1]['records']
    for lanes in (3, 64):
        for c, a, b in zip(IB.corpus(), one, host['runs'][lanes]['records']):
            for key in ('cand', 'words', 'chain', 'window_crc', 'words2'):
                assert np.array_equal(a[key], b[key]), (lanes, c['name'], key)
            assert a['chain_ok'] == b['chain_ok'] and a['out'] == b['out'], (lanes, c['name'])


def test_truncations_and_bit_flips_end_with_an_error_a_crc_mismatch_or_the_right_bytes(host):
    last = host['runs'][1]['last']
    print(last)
    damaged, right = int(re.search(r'damaged (\d+)', last).group(1)), int(re.search(r'damaged_right (\d+)', last).group(1))
    assert damaged == 128 * sum(1 for c in IB.corpus() if c['damage']) and damaged >= 4 * 128
    assert right < damaged // 8                                              # (a flip in padding bits changes nothing)
    # with lanes: the striped copies on damaged input
    cases = [(c['comp'], c['want']) for c in IB.corpus() if c['damage']][:2]
    for lanes in (3, 64):
        _, stdout = IB.run_host_check(host['exe'], cases, host['tmp'], tag='ib_damage_%d' % lanes, mode=[1] * len(cases), lanes=lanes)
        assert stdout.strip().splitlines()[-1].endswith('mismatches 0'), stdout[-3000:]


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def test_foreign_rule_keyword_over_environment_over_default(monkeypatch):
    assert loadz.FOREIGN_ENV == 'VARSEP_NPZ_FOREIGN'
    monkeypatch.delenv(loadz.FOREIGN_ENV, raising=False)
    assert loadz.npz_foreign() == 'host' and loadz.npz_foreign(None) == 'host'
    monkeypatch.setenv(loadz.FOREIGN_ENV, '')
    assert loadz.npz_foreign() == 'host'                                    # empty counts as unset
    for env in ('host', 'device'):
        monkeypatch.setenv(loadz.FOREIGN_ENV, env)
        assert loadz.npz_foreign() == env
        for kw in ('host', 'device'):
            assert loadz.npz_foreign(kw) == kw                              # the keyword over the environment
    monkeypatch.setenv(loadz.FOREIGN_ENV, 'gpu')
    with pytest.raises(ValueError, match=r"VARSEP_NPZ_FOREIGN='gpu'.*'host' or 'device'"):
        loadz.npz_foreign()
    assert loadz.npz_foreign('device') == 'device'
    with pytest.raises(ValueError, match=r"foreign='blocks'.*'host' or 'device'"):
        loadz.npz_foreign('blocks')


def _stand_ins(monkeypatch, calls):
    """ops.inflate_raw says `not chunked`, ops.inflate_blocks inflates with host zlib: the rule's wiring without a GPU."""
    monkeypatch.setattr(ops, 'crc32', lambda t, init=0: zlib.crc32(t.numpy().tobytes(), init))
    monkeypatch.setattr(ops, 'inflate_raw', lambda comp, n, crc=None, **k: ops.InflateNotChunked('stand-in'))

    def blocks(comp, n, crc=None, **k):
        calls.append(n)
        data = zlib.decompress(comp.numpy().tobytes(), -15)
        if len(data) > 100000:
            return ops.InflateNotChunked('too long for the stand-in')
        return torch.from_numpy(np.frombuffer(data, np.uint8).copy())

    monkeypatch.setattr(ops, 'inflate_blocks', blocks)


def test_load_sends_foreign_members_where_the_rule_says(tmp_path, monkeypatch):
    arrays = dict(a=np.arange(5000, dtype=np.int32).reshape(50, 100), b=np.array(2.5), big=np.arange(30000, dtype=np.int64),
                  f=np.asfortranarray(np.arange(12.).reshape(3, 4)))
    path = str(tmp_path / 'x.npz')
    np.savez_compressed(path, **arrays)
    calls = []
    _stand_ins(monkeypatch, calls)
    monkeypatch.delenv(loadz.FOREIGN_ENV, raising=False)
    report = {}
    got = loadz.load(path, 'cpu', load='device', foreign='device', report=report)
    assert report['a'] == report['b'] == ('device', 'chained at its block headers') and len(calls) == 3
    assert report['big'] == ('host', 'not chunked: too long for the stand-in')   # the second refusal's reason, and the host route
    assert report['f'] == ('host', 'Fortran order')
    for k, v in arrays.items():
        assert np.array_equal(got[k].numpy(), v) and got[k].numpy().dtype == v.dtype, k
    # the environment, and the keyword over it
    del calls[:]
    monkeypatch.setenv(loadz.FOREIGN_ENV, 'device')
    report = {}
    loadz.load(path, 'cpu', keys=('a',), load='device', report=report)
    assert report['a'][0] == 'device' and len(calls) == 1
    loadz.load(path, 'cpu', keys=('a',), load='device', foreign='host', report=report)
    assert report['a'] == ('host', 'not chunked: stand-in') and len(calls) == 1
    monkeypatch.setenv(loadz.FOREIGN_ENV, 'both')
    with pytest.raises(ValueError, match='VARSEP_NPZ_FOREIGN'):
        loadz.load(path, 'cpu', load='device')
    with pytest.raises(ValueError, match="foreign='gpu'"):
        loadz.load(path, 'cpu', load='device', foreign='gpu')


@pytest.mark.parametrize('env', [None, '', 'host'])
def test_with_foreign_host_inflate_blocks_is_never_called(tmp_path, monkeypatch, env):
    arrays = dict(a=np.arange(5000, dtype=np.int32), b=np.array(True))
    path = str(tmp_path / 'x.npz')
    np.savez_compressed(path, **arrays)
    _stand_ins(monkeypatch, [])
    monkeypatch.setattr(ops, 'inflate_blocks', lambda *a, **k: pytest.fail('the block-parallel reader is opt-in'))
    if env is None:
        monkeypatch.delenv(loadz.FOREIGN_ENV, raising=False)
    else:
        monkeypatch.setenv(loadz.FOREIGN_ENV, env)
    for kwargs in (dict(), dict(foreign='host')):
        report = {}
        got = loadz.load(path, 'cpu', load='device', report=report, **kwargs)
        assert all(report[k] == ('host', 'not chunked: stand-in') for k in arrays)
        assert all(np.array_equal(got[k].numpy(), v) for k, v in arrays.items())
    monkeypatch.setenv(loadz.FOREIGN_ENV, 'device')
    loadz.load(path, 'cpu', load='host')                                    # the rule matters only when the loader is `device`
    loadz.load(path, 'cpu', load='device', foreign='host')


def test_the_rule_reaches_make_dataset_and_load_dataset(tmp_path, monkeypatch):
    from spatiotemporal_variable_separation_amd.test.mnist import test as mnist_test
    rs = np.random.RandomState(3)
    sequences = rs.randint(0, 256, size=(6, 5, 1, 64, 64)).astype(np.uint8)
    np.savez_compressed(os.path.join(str(tmp_path), 'mmnist_test_2digits_64.npz'), sequences=sequences)
    asked = []

    def stand_in(path, device, keys=None, load=None, report=None, **extra):
        asked.append((load, extra))
        with np.load(path) as z:
            return {k: torch.from_numpy(z[k]) for k in keys}

    monkeypatch.setattr(loadz, 'load', stand_in)
    monkeypatch.setattr(ops, 'u8_tn_to_f32_nt', lambda x: x.transpose(0, 1).to(torch.float32).contiguous())
    want = torch.from_numpy(sequences.swapaxes(0, 1).astype(np.float32))
    args = type('Args', (), dict(data_dir=str(tmp_path), nt_cond=2, nt_pred=4, n_object=2))()

    def make(**kwargs):
        return moving_mnist.MovingMNIST.make_dataset(str(tmp_path), 64, 2, 6, 4, True, 2, False, device='cpu', **kwargs).data

    monkeypatch.setenv(loadz.LOAD_ENV, 'device')
    monkeypatch.delenv(loadz.FOREIGN_ENV, raising=False)
    assert torch.equal(make(), want) and asked == [('device', {})]            # nothing set: the call is the one of before
    monkeypatch.setenv(loadz.FOREIGN_ENV, 'device')
    del asked[:]
    assert torch.equal(make(), want) and torch.equal(make(foreign='host'), want)
    assert torch.equal(mnist_test.load_dataset(args, train=False, device='cpu').data, want)
    assert torch.equal(mnist_test.load_dataset(args, train=False, device='cpu', load='device', foreign='host').data, want)
    assert asked == [('device', {'foreign': 'device'}), ('device', {'foreign': 'host'}), ('device', {'foreign': 'device'}), ('device', {'foreign': 'host'})]
    del asked[:]
    monkeypatch.setenv(loadz.LOAD_ENV, 'host')
    assert torch.equal(make(), want) and asked == []                        # the loader is `host`: the second rule changes nothing
    monkeypatch.setenv(loadz.FOREIGN_ENV, 'gpu')
    with pytest.raises(ValueError, match='VARSEP_NPZ_FOREIGN'):
        make()

"""The stored-block finder of the block-parallel .npz reader, the part that needs no GPU: the declaration and argument checks of
vs_inflate_block_scan_stored; the candidate rule of csrc/vs_inflate_blocks_core.h (vsb_stored_boundary, vsb_stored_start) compiled for the
host against its Python restatement and against a block walker that is not the code under test; the whole route with both finders --
scan, probe, chain, windows, decode -- on the corpus of tests/inflate_stored_inputs.py and on the existing corpus, with one lane and with
threads playing 3 and 64 lanes, on truncations and bit flips; and the rule VARSEP_NPZ_FINDER that switches the finder on."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest
import torch

import deflate_inputs as D
import inflate_blocks_inputs as IB
import inflate_stored_inputs as IS
from spatiotemporal_variable_separation_amd import _lib, ops
from spatiotemporal_variable_separation_amd.data import moving_mnist
from spatiotemporal_variable_separation_amd.utils import loadz

ENTRY = 'vs_inflate_block_scan_stored'


# ---- the entry point ---------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_built():
    header = open(os.path.join(D.ROOT, 'include', 'varsep_hip.h')).read()
    lib = _lib.load_library()
    assert re.search(r'\bint %s\(' % ENTRY, header) and ENTRY in _lib.SIGNATURES and hasattr(lib, ENTRY)
    declared = re.search(r'\bint %s\(([^;]*)\);' % ENTRY, header).group(1)
    assert len(declared.split(',')) == len(_lib.SIGNATURES[ENTRY][1])
    assert _lib.SIGNATURES[ENTRY] == _lib.SIGNATURES['vs_inflate_block_scan']   # the count-then-list contract of the dynamic scan


def test_entry_point_refuses_null_pointers_negative_sizes_and_a_null_list_with_room():
    lib = _lib.load_library()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def scan(comp=p, n=16, cand=p, cap=4, count=p):
        return lib.vs_inflate_block_scan_stored(comp, n, cand, cap, count, None)

    for kwargs in (dict(comp=None), dict(count=None), dict(cand=None), dict(cand=None, cap=1), dict(n=-1), dict(cap=-1), dict(n=(1 << 31) * 1024)):
        assert scan(**kwargs) == -1, kwargs
        assert lib.vs_last_error().decode().startswith(ENTRY + ':'), kwargs
    # a stream with no room for LEN, NLEN and one more byte: nothing to find, nothing launched
    assert scan(n=0) == 0 and scan(n=4) == 0 and scan(n=3, cand=None, cap=0) == 0
    assert all(v == 0 for v in buf)


def test_ops_refuse_host_tensors():
    with pytest.raises(_lib.VarsepHipError):
        ops.inflate_block_scan(torch.zeros(10, dtype=torch.uint8), stored=True)
    with pytest.raises(_lib.VarsepHipError):
        ops.inflate_blocks(torch.zeros(10, dtype=torch.uint8), 10, stored=True)


# ---- the rule, restated, on small streams ------------------------------------------------------------------------------------------
def test_the_restatement_on_hand_made_streams():
    marker = bytes([0x00, 0x00, 0xff, 0xff])
    assert IS.stored_candidates(b'') == IS.stored_candidates(marker) == []      # B + 4 + LEN < n is strict
    assert IS.stored_candidates(marker + b'\x03') == []                        # B = 0: every q is negative
    assert IS.stored_candidates(b'\x00' + marker + b'\x03') == [0, 1, 2, 3, 4, 5]   # B = 1: k = 0 .. 5, q = 5 .. 0
    assert IS.stored_candidates(b'\x01' + marker + b'\x03') == [1, 2, 3, 4, 5]
    assert IS.stored_candidates(b'\x80' + marker + b'\x03') == []              # a one straight in front of the boundary
    assert IS.stored_candidates(b'\xff\x1f' + marker + b'\x03') == [13]       # three zero bits: k = 0 alone
    assert IS.stored_candidates(b'\xff\x3f' + marker + b'\x03') == []
    assert IS.stored_candidates(b'\x55\x00\x00' + marker + b'\x03') == list(range(14, 22))   # B = 3 behind 16 zero bits: all eight, no ninth
    assert IS.stored_candidates(b'\x00\x02\x00\xfd\xff' + b'ab') == []          # LEN = 2 and two bytes behind it: a final block at best
    assert IS.stored_candidates(b'\x00\x02\x00\xfd\xff' + b'abc') == [0, 1, 2, 3, 4, 5]


# ---- the logic on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """The stored host build (both finders) on the new corpus with 1, 3 and 64 lanes and on the existing corpus with one lane; the
    existing host build (the dynamic finder alone: the list the union is checked against, and the verdict of before) on both with one lane."""
    tmp = tmp_path_factory.mktemp('inflate_stored_host')
    corpus, old = IS.corpus(), IB.corpus()
    exe, sanitized = IS.compile_host_check(tmp)
    cases = [(c['comp'], c['want']) for c in corpus]
    runs = {}
    for lanes in (1, 3, 64):
        records, stdout = IS.run_host_check(exe, cases, tmp, tag='is_%d' % lanes, lanes=lanes)
        last = stdout.strip().splitlines()[-1]
        print('sanitizers:', sanitized, '|', last)
        assert last.startswith('lanes %d ' % lanes) and last.endswith('mismatches 0'), stdout[-3000:]
        runs[lanes] = records
    on_old, stdout = IS.run_host_check(exe, [(c['comp'], c['want']) for c in old], tmp, tag='is_old')
    assert stdout.strip().splitlines()[-1].endswith('mismatches 0'), stdout[-3000:]
    exe_dynamic, _ = IB.compile_host_check(tmp)
    dynamic_only, stdout = IB.run_host_check(exe_dynamic, cases, tmp, tag='ib_new')
    assert stdout.strip().splitlines()[-1].endswith('mismatches 0'), stdout[-3000:]
    old_dynamic, stdout = IB.run_host_check(exe_dynamic, [(c['comp'], c['want']) for c in old], tmp, tag='ib_old')
    assert stdout.strip().splitlines()[-1].endswith('mismatches 0'), stdout[-3000:]
    return dict(tmp=tmp, exe=exe, runs=runs, cases={c['name']: (c, r, d) for c, r, d in zip(corpus, runs[1], dynamic_only)},
                old={c['name']: (c, r, d) for c, r, d in zip(old, on_old, old_dynamic)})


def test_the_corpus_is_what_it_claims_to_be(host):
    cases = host['cases']
    assert list(cases) == ['random_above_cap', 'random_level0_above_cap', 'text_random_text', 'planted_stored', 'sync_flushed', 'stored_small']
    for name, (c, r, d) in cases.items():
        z = zlib.decompressobj(-15)
        assert z.decompress(c['comp']) == c['want'] and z.eof and not z.unused_data, name
        blocks, claims = IB.walk_blocks(c['comp']), c['claims']
        stored = [b for b in blocks if b['type'] == 0]
        dynamic = [b for b in blocks if b['type'] == 2]
        print(name, 'bytes', len(c['want']), 'compressed', len(c['comp']), 'stored/dynamic/all', len(stored), len(dynamic), len(blocks),
              'candidates', len(r['cand']), 'of them dynamic', len(d['cand']))
        assert [b['end'] for b in blocks[:-1]] == [b['start'] for b in blocks[1:]] and blocks[0]['start'] == 0 and blocks[-1]['final'], name
        if claims.get('only_stored'):
            assert len(stored) == len(blocks) and len(d['cand']) == 1, name
        assert len(c['comp']) >= claims.get('min_comp', 0) and len(dynamic) >= claims.get('min_dynamic', 0), name
        if 'stored_len' in claims:                                          # blocks of 65 535 bytes (where zlib's input buffer ran out, shorter ones)
            sizes = [(b['end'] - b['start']) // 8 for b in stored]
            assert max(sizes) == claims['stored_len'] + 5 and sum(1 for s in sizes if s == claims['stored_len'] + 5) >= 10, name
        if 'min_gap' in claims:                                             # more input than a span may read between two dynamic headers
            at = [b['start'] for b in dynamic]
            assert max(b - a for a, b in zip(at, at[1:])) > 8 * claims['min_gap'], name
        if 'min_empty_stored' in claims:
            assert sum(1 for b in stored if b['end'] - b['header_end'] < 8 + 32) >= claims['min_empty_stored'], name
        if 'planted' in claims:
            at, spots = c['comp'].find(claims['planted']), set()
            while at >= 0:
                spots.add(at + 2)
                at = c['comp'].find(claims['planted'], at + 1)
            starts = {(b['header_end'] + 7) // 8 for b in stored}
            assert len(spots) == IS.PLANTED and not spots & starts, name       # boundaries that are none
            assert spots <= set(IS.stored_boundaries(c['comp']).tolist()), name
            assert (r['words'][np.isin(r['cand'], [8 * B - 8 for B in spots]), 0] != 0).sum() >= 100, name   # probed, garbage, refused
    c, r, d = cases['stored_small']
    assert len(c['comp']) < 40000
    c, r, d = cases['text_random_text']
    assert len(c['comp']) > IB.MAX_IN and {b['type'] for b in IB.walk_blocks(c['comp'])} >= {0, 2}


def test_the_host_builds_stored_candidates_are_the_restatements_and_no_true_start_is_missed(host):
    total = true = 0
    for table in (host['cases'], host['old']):
        for name, (c, r, d) in table.items():
            cand = r['cand'].tolist()
            assert cand == sorted(set(cand)) and cand[0] == 0, name
            assert cand == IS.union_candidates(c['comp'], d['cand']), name     # exactly the rule's, on top of the dynamic finder's own list
            if table is host['old'] and not (c['claims'].get('only_stored') or c['claims'].get('min_stored')):
                continue                                                    # (the walker is slow; of the existing corpus, the streams with stored blocks)
            starts = {b['start'] for b in IB.walk_blocks(c['comp']) if b['type'] == 0 and not b['final']}
            assert starts - {0} <= set(cand), (name, sorted(starts - set(cand))[:5])
            if table is host['cases'] and name != 'planted_stored':
                total += len(IS.stored_candidates(c['comp']))
                true += len(starts)
    print('stored candidates', total, 'true non-final stored starts', true, 'candidates per true start %.2f' % (total / true))
    assert 5 <= total / true <= 8.5                                         # k = 0 .. 5 behind another stored block, 8 at the most; few chance boundaries


def test_every_new_case_chains_and_none_above_the_allowance_does_without_the_stored_finder(host):
    """With the dynamic list alone a stream chains when no span needs more than the allowance: `sync_flushed` (dynamic headers all along) and
    the two streams shorter than the allowance, which are one span from bit 0.  The three above it do not: that is what the finder is for."""
    for name, (c, r, d) in host['cases'].items():
        assert r['chain_ok'] and r['fail'] == 0 and r['out'] == c['want'], (name, r['fail'])
        assert d['chain_ok'] == c['dynamic_chains'] == (name in ('sync_flushed', 'planted_stored', 'stored_small')), (name, d['fail'])
        w = r['words'][r['chain']]
        assert (w[:, 0] == 0).all() and w[-1, 2] == 1 and (w[-1, 1] + 7) // 8 == len(c['comp']) and (w[:-1, 2] == 0).all(), name
        assert w[:, 3].sum() == len(c['want']) and (r['cand'][r['chain'][1:]] == w[:-1, 1]).all(), name
        assert (r['words2'] == w[:, [0, 1, 3]]).all(), name
        ends = np.cumsum(w[:, 3])
        data = bytes(IB.WINDOW) + c['want']
        for k in {0, len(w) // 2, len(w) - 1}:
            assert r['window_crc'][k + 1] == zlib.crc32(data[int(ends[k]):int(ends[k]) + IB.WINDOW]), (name, k)
    for name in ('random_above_cap', 'random_level0_above_cap', 'text_random_text'):
        c, r, d = host['cases'][name]
        assert (d['words'][:, 0] == IB.CAP_STATUS).any() and d['fail'] == 1, name   # today: a span hits its allowance, the host inflates
    c, r, d = host['cases']['random_above_cap']
    blocks = IB.walk_blocks(c['comp'])
    assert len(r['chain']) == len(blocks) - 1                               # every stored block is a span of its own; the final one is no candidate
    c, r, d = host['cases']['sync_flushed']
    assert len(r['chain']) > len(d['chain'])                                # the empty stored blocks cut spans the dynamic list runs through


def test_the_existing_corpus_gives_the_same_bytes_and_the_same_verdict_with_the_union_list(host):
    for name, (c, r, d) in host['old'].items():
        assert r['chain_ok'] == d['chain_ok'] == c['chains'], (name, r['fail'], d['fail'])
        assert r['out'] == d['out'] and (not r['chain_ok'] or r['out'] == c['want']), name
        assert set(d['cand'].tolist()) <= set(r['cand'].tolist()), name
    c, r, d = host['old']['fixed_above_cap']
    assert not r['chain_ok'] and r['fail'] == 1 and r['words'][0, 0] == IB.CAP_STATUS   # a fixed header cannot be found: still the host's


def test_threads_playing_3_and_64_lanes_give_the_one_lane_records(host):
    for lanes in (3, 64):
        for c, a, b in zip(IS.corpus(), host['runs'][1], host['runs'][lanes]):
            for key in ('cand', 'words', 'chain', 'window_crc', 'words2'):
                assert np.array_equal(a[key], b[key]), (lanes, c['name'], key)
            assert a['chain_ok'] == b['chain_ok'] and a['out'] == b['out'], (lanes, c['name'])


def test_truncations_and_bit_flips_end_without_a_chain_with_another_crc_or_with_the_right_bytes(host):
    """A flip inside the bytes of a stored block chains and gives other bytes: nothing in a DEFLATE stream can tell, the CRC-32 of the zip
    record does (ops.inflate_blocks(crc=...)); the program counts such a run as right only when the bytes are zlib's."""
    cases = IS.damage_cases()
    for lanes in (1, 3, 64):
        records, stdout = IS.run_host_check(host['exe'], cases, host['tmp'], tag='is_damage_%d' % lanes, mode=[1] * len(cases), lanes=lanes)
        last = stdout.strip().splitlines()[-1]
        print(last)
        assert last.endswith('mismatches 0'), stdout[-3000:]
        assert int(re.search(r'damaged (\d+)', last).group(1)) == 128 * len(cases)
        assert records[0]['chain_ok'] and not records[1]['chain_ok']        # a whole stream, and one that does not end


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def test_finder_rule_keyword_over_environment_over_default(monkeypatch):
    assert loadz.FINDER_ENV == 'VARSEP_NPZ_FINDER'
    monkeypatch.delenv(loadz.FINDER_ENV, raising=False)
    assert loadz.npz_finder() == 'dynamic' and loadz.npz_finder(None) == 'dynamic'
    monkeypatch.setenv(loadz.FINDER_ENV, '')
    assert loadz.npz_finder() == 'dynamic'                                  # empty counts as unset
    for env in ('dynamic', 'all'):
        monkeypatch.setenv(loadz.FINDER_ENV, env)
        assert loadz.npz_finder() == env
        for kw in ('dynamic', 'all'):
            assert loadz.npz_finder(kw) == kw                               # the keyword over the environment
    monkeypatch.setenv(loadz.FINDER_ENV, 'stored')
    with pytest.raises(ValueError, match=r"VARSEP_NPZ_FINDER='stored'.*'dynamic' or 'all'"):
        loadz.npz_finder()
    assert loadz.npz_finder('all') == 'all'
    with pytest.raises(ValueError, match=r"finder='both'.*'dynamic' or 'all'"):
        loadz.npz_finder('both')


def _stand_ins(monkeypatch, calls):
    """ops.inflate_raw says `not chunked`, ops.inflate_blocks inflates with host zlib and records its keywords: the wiring without a GPU."""
    monkeypatch.setattr(ops, 'crc32', lambda t, init=0: zlib.crc32(t.numpy().tobytes(), init))
    monkeypatch.setattr(ops, 'inflate_raw', lambda comp, n, crc=None, **k: ops.InflateNotChunked('stand-in'))

    def blocks(comp, n, crc=None, **k):
        calls.append(dict(k))
        return torch.from_numpy(np.frombuffer(zlib.decompress(comp.numpy().tobytes(), -15), np.uint8).copy())

    monkeypatch.setattr(ops, 'inflate_blocks', blocks)


def test_load_passes_stored_only_with_all(tmp_path, monkeypatch):
    arrays = dict(a=np.arange(5000, dtype=np.int32).reshape(50, 100), noise=np.random.RandomState(5).randint(0, 256, 9000).astype(np.uint8))
    path = str(tmp_path / 'x.npz')
    np.savez_compressed(path, **arrays)
    calls = []
    _stand_ins(monkeypatch, calls)
    monkeypatch.delenv(loadz.FOREIGN_ENV, raising=False)
    monkeypatch.delenv(loadz.FINDER_ENV, raising=False)

    def run(**kwargs):
        del calls[:]
        report = {}
        got = loadz.load(path, 'cpu', load='device', report=report, **kwargs)
        assert all(np.array_equal(got[k].numpy(), v) for k, v in arrays.items())
        return report, list(calls)

    report, seen = run(foreign='device')
    assert seen == [{}, {}] and report['a'] == report['noise'] == ('device', 'chained at its block headers')   # today's call, argument for argument
    report, seen = run(foreign='device', finder='dynamic')
    assert seen == [{}, {}]
    report, seen = run(foreign='device', finder='all')
    assert seen == [dict(stored=True)] * 2 and report['a'] == report['noise'] == ('device', 'chained at its block headers')
    monkeypatch.setenv(loadz.FINDER_ENV, 'all')                             # the environment, and the keyword over it
    assert run(foreign='device')[1] == [dict(stored=True)] * 2
    assert run(foreign='device', finder='dynamic')[1] == [{}, {}]
    report, seen = run()                                                    # the foreign rule says `host`: the finder is not asked
    assert seen == [] and report['a'] == ('host', 'not chunked: stand-in')
    loadz.load(path, 'cpu', load='host')
    monkeypatch.setenv(loadz.FINDER_ENV, 'both')
    with pytest.raises(ValueError, match='VARSEP_NPZ_FINDER'):
        loadz.load(path, 'cpu', load='device', foreign='device')
    with pytest.raises(ValueError, match="finder='stored'"):
        loadz.load(path, 'cpu', load='device', foreign='device', finder='stored')


def test_the_rule_reaches_make_dataset_and_load_dataset(tmp_path, monkeypatch):
    from spatiotemporal_variable_separation_amd.test.mnist import test as mnist_test
    sequences = np.random.RandomState(3).randint(0, 256, size=(6, 5, 1, 64, 64)).astype(np.uint8)
    np.savez_compressed(os.path.join(str(tmp_path), 'mmnist_test_2digits_64.npz'), sequences=sequences)
    asked = []

    def stand_in(path, device, keys=None, load=None, report=None, **extra):
        asked.append(extra)
        with np.load(path) as z:
            return {k: torch.from_numpy(z[k]) for k in keys}

    monkeypatch.setattr(loadz, 'load', stand_in)
    monkeypatch.setattr(ops, 'u8_tn_to_f32_nt', lambda x: x.transpose(0, 1).to(torch.float32).contiguous())
    args = type('Args', (), dict(data_dir=str(tmp_path), nt_cond=2, nt_pred=4, n_object=2))()

    def make(**kwargs):
        return moving_mnist.MovingMNIST.make_dataset(str(tmp_path), 64, 2, 6, 4, True, 2, False, device='cpu', **kwargs).data

    monkeypatch.setenv(loadz.LOAD_ENV, 'device')
    monkeypatch.setenv(loadz.FOREIGN_ENV, 'device')
    monkeypatch.delenv(loadz.FINDER_ENV, raising=False)
    make()
    assert asked == [{'foreign': 'device'}]                                 # nothing set: the call is the one of before
    del asked[:]
    monkeypatch.setenv(loadz.FINDER_ENV, 'all')
    make()
    make(finder='dynamic')
    mnist_test.load_dataset(args, train=False, device='cpu')
    mnist_test.load_dataset(args, train=False, device='cpu', finder='dynamic')
    assert asked == [{'foreign': 'device', 'finder': 'all'}, {'foreign': 'device', 'finder': 'dynamic'}, {'foreign': 'device', 'finder': 'all'},
                     {'foreign': 'device', 'finder': 'dynamic'}]
    monkeypatch.setenv(loadz.FINDER_ENV, 'stored')
    with pytest.raises(ValueError, match='VARSEP_NPZ_FINDER'):
        make()

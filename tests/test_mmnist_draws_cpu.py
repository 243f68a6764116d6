"""The Moving-MNIST training draws on the device, the part that needs no GPU: the entry point's declaration and argument checks, the logic of
the stream (csrc/vs_mt19937_core.h) compiled for the host and run on the cases of tests/mmnist_draws_inputs.py against NumPy itself -- once
as the header's one-lane form and once with threads playing 3, 64 and 256 lanes, the windowed and scanned form the kernel runs -- and the rule
by which `main` selects who draws."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mmnist_draws_inputs as MD
from spatiotemporal_variable_separation_amd import _lib, main as vs_main, ops

LANES = (3, 64, 256)             # an odd count that divides nothing, one wave, the kernel's workgroup


def test_entry_point_is_declared_bound_and_built():
    header = open(os.path.join(MD.ROOT, 'include', 'varsep_hip.h')).read()
    lib = _lib.load_library()
    assert re.search(r'\bint vs_mt19937_randint\(', header)
    assert 'vs_mt19937_randint' in _lib.SIGNATURES and hasattr(lib, 'vs_mt19937_randint')
    assert 'vs_mt19937.hip' in _lib.SOURCES
    for macro, value in (('VS_MT19937_STATE_WORDS', ops.MT19937_STATE_WORDS), ('VS_MT19937_MAX_COLS', ops.MT19937_MAX_COLS)):
        assert re.search(r'#define %s %d\b' % (macro, value), header), macro
    assert (ops.MT19937_STATE_WORDS, ops.MT19937_MAX_COLS) == (MD.STATE_WORDS, MD.MAX_COLS) == (625, 8)


def test_entry_point_refuses_null_pointers_and_bad_sizes():
    lib = _lib.load_library()
    buf = (ctypes.c_int32 * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def cols(values):
        return (ctypes.c_int32 * 9)(*(list(values) + [0] * (9 - len(values))))

    lows, highs = cols([0, 0, -4]), cols([256, 37, 5])

    def call(state=p, lows=lows, highs=highs, k=3, n_rows=4, out=p, bad=None):
        return lib.vs_mt19937_randint(state, lows, highs, k, n_rows, out, bad, None)

    for kwargs in (dict(state=None), dict(lows=None), dict(highs=None), dict(out=None), dict(k=0), dict(k=9), dict(k=-1), dict(n_rows=-1),
                   dict(n_rows=(1 << 40) + 1), dict(highs=cols([256, 0, 5])), dict(highs=cols([256, 37, -4])), dict(lows=cols([0, 0, 5])),
                   dict(lows=cols([0] * 8), highs=cols([1] * 7 + [0]), k=8)):
        assert call(**kwargs) == -1, kwargs
        assert 'vs_mt19937_randint' in lib.vs_last_error().decode(), kwargs
    call(highs=cols([256, 37, -4]))
    assert 'column 2' in lib.vs_last_error().decode() and '-4' in lib.vs_last_error().decode()
    assert call(n_rows=0) == 0                                              # nothing to do, nothing launched
    assert call(n_rows=0, highs=cols([256, 0, 5])) == -1                    # the columns are checked all the same


def test_op_refuses_cpu_tensors_and_malformed_operands(monkeypatch):
    state = torch.zeros(625, dtype=torch.int32)
    with pytest.raises(_lib.VarsepHipError, match='MI355X'):
        ops.mt19937_randint(state, [0], [2], 3)
    monkeypatch.setattr(ops, 'require_cuda', lambda *t: None)               # past the device check, still on the host: nothing is launched
    for bad_state in (torch.zeros(624, dtype=torch.int32), torch.zeros(625, dtype=torch.int64), torch.zeros(1250, dtype=torch.int32)[::2],
                      torch.zeros((625, 1), dtype=torch.int32)):
        with pytest.raises(_lib.VarsepHipError, match='state'):
            ops.mt19937_randint(bad_state, [0], [2], 3)
    with pytest.raises(_lib.VarsepHipError, match='lows and highs'):
        ops.mt19937_randint(state, [0, 0], [2], 3)
    with pytest.raises(_lib.VarsepHipError, match='lows and highs'):
        ops.mt19937_randint(state, [0], [2 ** 31], 3)
    with pytest.raises(_lib.VarsepHipError, match='negative'):
        ops.mt19937_randint(state, [0], [2], -1)
    for out in (torch.zeros((3, 2), dtype=torch.int32), torch.zeros((3, 1), dtype=torch.int64), torch.zeros((3, 2), dtype=torch.int32)[:, :1]):
        with pytest.raises(_lib.VarsepHipError, match='out'):
            ops.mt19937_randint(state, [0], [2], 3, out=out)
    with pytest.raises(_lib.VarsepHipError, match='low 2 >= high 2'):       # refused by the entry point, also when there is nothing to draw
        ops.mt19937_randint(state, [2], [2], 0)
    with pytest.raises(_lib.VarsepHipError, match='k 9'):
        ops.mt19937_randint(state, [0] * 9, [2] * 9, 0)
    empty = ops.mt19937_randint(state, [0, 5], [2, 6], 0)
    assert empty.shape == (0, 2) and empty.dtype == torch.int32 and not state.any()


def test_device_random_state_refuses_a_cpu_device_and_leaves_the_global_stream():
    from spatiotemporal_variable_separation_amd.data.numpy_stream import DeviceRandomState
    before = np.random.get_state()
    rs = DeviceRandomState(None, 'cpu')                                     # the upload is a copy; no launch yet
    after = np.random.get_state()
    assert before[2] == after[2] and np.array_equal(before[1], after[1])
    got = rs.get_state()
    assert got[0] == 'MT19937' and np.array_equal(got[1], before[1]) and got[2:] == before[2:]
    with pytest.raises(_lib.VarsepHipError, match='MI355X'):
        rs.randint_table([0], [2], 3)
    source = np.random.RandomState(5)
    source.standard_normal(3)                                               # an odd count: a Gaussian is cached
    st = source.get_state()
    assert st[3] == 1
    kept = DeviceRandomState(source, 'cpu').to_random_state()
    assert kept.get_state()[3:] == st[3:] and kept.standard_normal() == source.standard_normal() and kept.randint(0, 99) == source.randint(0, 99)


# ---- the stream's logic on the host --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """{lanes: {name: (statuses, tables, state words)}} of the host builds: 1 is the header's own one-lane form, the others are threads."""
    tmp = tmp_path_factory.mktemp('mt19937_host')
    plain, sanitized = MD.compile_host_check(tmp)
    lanes, lanes_sanitized = MD.compile_host_check(tmp, lanes=True)
    print('sanitizers: plain', sanitized, '| lanes', lanes_sanitized)
    out = {1: MD.run_host_check(plain, MD.cases(), tmp, lanes=1)}
    for n in LANES:
        out[n] = MD.run_host_check(lanes, MD.cases(), tmp, lanes=n)
    return out


def test_cases_hold_what_the_stream_can_get_wrong():
    c = {x['name']: x for x in MD.cases()}
    assert sorted(int(c['start_pos_%d' % p]['state'][MD.N]) for p in MD.START_POSITIONS) == [0, 1, 227, 396, 397, 623, 624]
    tables, words = MD.numpy_results()['ends_on_624']
    assert int(words[MD.N]) == 624 and np.array_equal(words[:MD.N], c['ends_on_624']['state'][:MD.N])      # NumPy keeps the old key
    assert not np.array_equal(MD.numpy_results()['ends_on_624_then_goes_on'][1][:MD.N], words[:MD.N])        # and twists on the next draw
    assert c['two_regenerations']['calls'] == [1300] and int(c['two_regenerations']['state'][MD.N]) + 1300 > 2 * 624
    assert [c['product_B%d_nd%d' % bn]['calls'] for bn in ((1, 1), (3, 2), (128, 2))] == [[1], [6], [256]]
    assert c['product_B128_nd2']['cols'] == MD.product_cols() and len(MD.product_cols()) == 5
    rng = {n: [b - 1 - a for a, b in c[n]['cols']] for n in c}
    assert rng['rng0_alone'] == [0] and set(rng['rng0_every_column']) == {0} and 0 in rng['rng0_mixed_in'] and any(rng['rng0_mixed_in'])
    assert all(r & (r + 1) == 0 for r in rng['never_rejects']) and all(r & (r - 1) == 0 for r in rng['rejects_half'])
    assert all(a < 0 for a, _ in c['negative_lows']['cols']) and len(c['k1']['cols']) == 1 and len(c['k8']['cols']) == 8
    assert rng['wide_full'] == [2 ** 32 - 2] and rng['wide_positive'] == [2 ** 31 - 2]
    assert sum(c['back_to_back']['calls']) == c['back_to_back_summed']['calls'][0] and 0 in c['zero_rows']['calls']
    # a batch of 128 x 2 uses about 8 outputs per digit and crosses three or four regenerations
    words = MD.numpy_results()['product_B128_nd2'][1]
    assert MD.numpy_results()['product_B128_nd2'][0][0].shape == (256, 5)
    assert not np.array_equal(words[:MD.N], c['product_B128_nd2']['state'][:MD.N])


@pytest.mark.parametrize('lanes', (1,) + LANES)
def test_core_on_the_host_equals_numpy_on_every_case(host, lanes):
    want = MD.numpy_results()
    for c in MD.cases():
        statuses, tables, words = host[lanes][c['name']]
        ref_tables, ref_words = want[c['name']]
        assert statuses == [0] * len(c['calls']), (c['name'], statuses)
        for call, (got, ref) in enumerate(zip(tables, ref_tables)):
            assert got.shape == ref.shape and np.array_equal(got, ref), (c['name'], call)
        assert int(words[MD.N]) == int(ref_words[MD.N]), (c['name'], 'pos')
        assert np.array_equal(words[:MD.N], ref_words[:MD.N]), (c['name'], 'key')


def test_core_on_the_host_consumes_nothing_for_zero_ranges_and_splits_like_one_call(host):
    for lanes in (1,) + LANES:
        got = host[lanes]
        assert np.array_equal(got['rng0_every_column'][2], MD.case('rng0_every_column')['state'])
        assert np.array_equal(got['rng0_alone'][2], MD.case('rng0_alone')['state'])
        assert np.array_equal(got['rng0_every_column'][1][0], np.tile([5, 0, -3], (9, 1)))
        assert np.array_equal(np.concatenate(got['back_to_back'][1]), got['back_to_back_summed'][1][0])
        assert np.array_equal(got['back_to_back'][2], got['back_to_back_summed'][2])
        assert [t.shape for t in got['zero_rows'][1]] == [(0, 5), (4, 5), (0, 5)]
        assert int(got['ends_on_624'][2][MD.N]) == 624
        assert np.array_equal(got['ends_on_624'][2][:MD.N], MD.case('ends_on_624')['state'][:MD.N])          # the old key came back


def test_core_on_the_host_refuses_a_position_past_the_block(host, tmp_path):
    exe, _ = MD.compile_host_check(tmp_path)
    state = MD.start_state(9, 625)
    bad = dict(name='pos_625', state=state, cols=MD.product_cols(), calls=[4])
    statuses, tables, words = MD.run_host_check(exe, [bad], tmp_path, tag='bad')['pos_625']
    assert statuses == [1] and tables == [None] and np.array_equal(words, state)


# ---- who draws -------------------------------------------------------------------------------------------------------------------------
class _FakeDeviceRandomState:
    def __init__(self, source, device):
        self.source, self.device = source, device


class _FakeSet:
    rng = None

    def __len__(self):
        return 200000


def _loader(monkeypatch, world, rank=0, seed=3):
    from spatiotemporal_variable_separation_amd.data import numpy_stream
    monkeypatch.setattr(numpy_stream, 'DeviceRandomState', _FakeDeviceRandomState)
    train_set = _FakeSet()
    loader = vs_main.moving_mnist_loader(train_set, 8, seed, rank, world, 'cuda:0')
    return train_set, loader


def test_draws_rule_unset_host_device_and_a_bad_value(monkeypatch):
    assert vs_main.DRAWS_ENV == 'VARSEP_MMNIST_DRAWS'
    monkeypatch.delenv(vs_main.DRAWS_ENV, raising=False)
    assert vs_main.mmnist_draws() == 'host'
    monkeypatch.setenv(vs_main.DRAWS_ENV, '')
    assert vs_main.mmnist_draws() == 'host'                                 # empty counts as unset
    for value in ('host', 'device'):
        monkeypatch.setenv(vs_main.DRAWS_ENV, value)
        assert vs_main.mmnist_draws() == value
    monkeypatch.setenv(vs_main.DRAWS_ENV, 'gpu')
    with pytest.raises(ValueError, match=r"VARSEP_MMNIST_DRAWS='gpu'.*'host' or 'device'"):
        vs_main.mmnist_draws()
    with pytest.raises(ValueError, match='VARSEP_MMNIST_DRAWS'):            # refused before a loader exists
        _loader(monkeypatch, 1)


def test_default_stream_of_the_training_set_is_unchanged(monkeypatch):
    for env in (None, '', 'host'):
        if env is None:
            monkeypatch.delenv(vs_main.DRAWS_ENV, raising=False)
        else:
            monkeypatch.setenv(vs_main.DRAWS_ENV, env)
        train_set, loader = _loader(monkeypatch, world=1)
        assert train_set.rng is None and loader.dataset is train_set and loader.batch_size == 8      # the global NumPy stream
        for rank in (0, 1):
            train_set, loader = _loader(monkeypatch, world=2, rank=rank, seed=3)
            assert isinstance(train_set.rng, np.random.RandomState)
            want = np.random.RandomState(3 + 7919 * (rank + 1)).get_state()
            assert np.array_equal(train_set.rng.get_state()[1], want[1]) and train_set.rng.get_state()[2] == want[2]
            assert loader.n_items == 100000


def test_device_route_gives_every_rank_its_private_stream_on_the_device(monkeypatch):
    monkeypatch.setenv(vs_main.DRAWS_ENV, 'device')
    monkeypatch.setenv('VARSEP_MMNIST_EPOCH_LEN', '32')
    for world, rank in ((1, 0), (2, 0), (2, 1)):
        train_set, loader = _loader(monkeypatch, world=world, rank=rank, seed=3)
        assert isinstance(train_set.rng, _FakeDeviceRandomState) and train_set.rng.device == 'cuda:0'
        want = np.random.RandomState(3 + 7919 * (rank + 1)).get_state()
        got = train_set.rng.source.get_state()
        assert np.array_equal(got[1], want[1]) and got[2] == want[2]
        assert loader.n_items == 32 // world

"""The stochastic Moving-MNIST trajectories on the device, the part that needs no GPU: the entry point's declaration and argument checks, the
walk's logic (csrc/vs_mmnist_walk_core.h) compiled for the host and run on the cases of tests/smnist_inputs.py against the fixture written from
the reference's own sampler and against the NumPy-driven restatement -- once as the core's one-lane form and once as the lanes form with
threads playing 3, 64 and 256 lanes, the speculative form the kernel runs --, the host route of `MovingMNIST.draw_stochastic`, and the flag."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import smnist_inputs as SI
from mmnist_draws_inputs import N, ROOT, random_state_at, start_state, state_words
from oracle import mmnist_ref
from spatiotemporal_variable_separation_amd import _lib, main as vs_main, ops, options
from spatiotemporal_variable_separation_amd.data import moving_mnist
from spatiotemporal_variable_separation_amd.data.moving_mnist import MovingMNIST

LANES = (3, 64, 256)             # an odd count that divides nothing, one wave, four waves
NAME = 'vs_mmnist_stochastic_trajectories'


def test_entry_point_is_declared_bound_and_built():
    header = open(os.path.join(ROOT, 'include', 'varsep_hip.h')).read()
    lib = _lib.load_library()
    assert re.search(r'\bint %s\(' % NAME, header)
    assert NAME in _lib.SIGNATURES and hasattr(lib, NAME)
    assert 'vs_mmnist_walk.hip' in _lib.SOURCES
    assert re.search(r'#define VS_MMNIST_WALK_MAX_PRE %d\b' % ops.MMNIST_WALK_MAX_PRE, header)
    core = open(os.path.join(ROOT, 'spatiotemporal_variable_separation_amd', 'csrc', 'vs_mmnist_walk_core.h')).read()
    assert re.search(r'#define VSW_STATUS_BOUNCE 3\b', core) and re.search(r'#define VS_MMNIST_WALK_STATUS_BOUNCE 3\b', header)
    assert sorted(ops.MMNIST_WALK_STATUS) == [1, 2, 3]                      # the stream's two and the bounce budget, all distinct


def test_entry_point_refuses_null_pointers_and_bad_sizes():
    lib = _lib.load_library()
    buf = (ctypes.c_int32 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def cols(values):
        return (ctypes.c_int32 * 5)(*(list(values) + [0] * (5 - len(values))))

    lows, highs = cols([0, 0, 0, -4, -4]), cols([256, 37, 37, 5, 5])

    def call(state=p, lows=lows, highs=highs, n_pre=5, n_traj=4, seq_len=3, x_max=36, y_max=36, max_speed=4, start=None, pre=p, positions=p,
             latents=None, desc=None, nd=0):
        return getattr(lib, NAME)(state, lows, highs, n_pre, n_traj, seq_len, x_max, y_max, max_speed, start, pre, positions, latents, desc, nd,
                                  None, None)

    for kwargs in (dict(state=None), dict(lows=None), dict(highs=None), dict(pre=None), dict(positions=None), dict(n_pre=-1), dict(n_pre=6),
                   dict(n_pre=3), dict(n_pre=0), dict(seq_len=0), dict(seq_len=-2), dict(n_traj=-1), dict(n_traj=(1 << 24) + 1), dict(x_max=0),
                   dict(y_max=0), dict(x_max=-3), dict(max_speed=-1), dict(highs=cols([256, 0, 37, 5, 5])), dict(lows=cols([0, 0, 0, 5, -4])),
                   dict(desc=p, nd=0), dict(desc=p, nd=3), dict(desc=p, nd=9), dict(desc=p, nd=2, n_pre=4)):
        assert call(**kwargs) == -1, kwargs
        assert NAME in lib.vs_last_error().decode(), kwargs
    call(lows=cols([0, 0, 0, 5, -4]))
    assert 'column 3' in lib.vs_last_error().decode()
    assert call(n_traj=0) == 0                                              # nothing to do, nothing launched
    assert call(n_traj=0, n_pre=0, start=p, pre=None) == 0
    assert call(n_traj=0, x_max=0) == -1                                    # the arguments are checked all the same


def test_op_refuses_cpu_tensors_and_malformed_operands(monkeypatch):
    state = torch.zeros(625, dtype=torch.int32)
    lows, highs = (0, 0, 0, -4, -4), (256, 37, 37, 5, 5)
    with pytest.raises(_lib.VarsepHipError, match='MI355X'):
        ops.mmnist_stochastic_trajectories(state, 3, 15, lows, highs, 36, 36, 4)
    monkeypatch.setattr(ops, 'require_cuda', lambda *t: None)               # past the device check, still on the host: nothing is launched
    for bad_state in (torch.zeros(624, dtype=torch.int32), torch.zeros(625, dtype=torch.int64), torch.zeros(1250, dtype=torch.int32)[::2],
                      torch.zeros((625, 1), dtype=torch.int32)):
        with pytest.raises(_lib.VarsepHipError, match='state'):
            ops.mmnist_stochastic_trajectories(bad_state, 3, 15, lows, highs, 36, 36, 4)
    for bad_lows, bad_highs in ((lows[:4], highs), (lows + (0,), highs + (1,)), (lows, highs[:4] + (2 ** 31,))):
        with pytest.raises(_lib.VarsepHipError, match='lows and highs'):
            ops.mmnist_stochastic_trajectories(state, 3, 15, bad_lows, bad_highs, 36, 36, 4)
    for kwargs in (dict(n_traj=-1), dict(seq_len=0)):
        with pytest.raises(_lib.VarsepHipError, match='n_traj'):
            ops.mmnist_stochastic_trajectories(state, kwargs.get('n_traj', 3), kwargs.get('seq_len', 15), lows, highs, 36, 36, 4)
    for x_max, y_max, speed in ((0, 36, 4), (36, 0, 4), (36, 36, -1)):
        with pytest.raises(_lib.VarsepHipError, match='fills the frame'):
            ops.mmnist_stochastic_trajectories(state, 3, 15, lows, highs, x_max, y_max, speed)
    for start in (None, torch.zeros((3, 4), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.int32), torch.zeros((3, 8), dtype=torch.int32)[:, ::2]):
        with pytest.raises(_lib.VarsepHipError, match='start'):
            ops.mmnist_stochastic_trajectories(state, 3, 15, (), (), 36, 36, 4, start=start)
    for nd, n_pre in ((4, 5), (0, 5), (9, 5), (2, 4)):
        with pytest.raises(_lib.VarsepHipError, match='desc'):
            ops.mmnist_stochastic_trajectories(state, 6, 15, lows[5 - n_pre:], highs[5 - n_pre:], 36, 36, 4, desc_nd=nd)
    with pytest.raises(_lib.VarsepHipError, match='low 5 >= high 5'):       # refused by the entry point, also when there is nothing to walk
        ops.mmnist_stochastic_trajectories(state, 0, 15, (0, 0, 0, 5, -4), highs, 36, 36, 4)
    pre, positions, latents, desc = ops.mmnist_stochastic_trajectories(state, 0, 15, lows, highs, 36, 36, 4, latents=True, desc_nd=2)
    assert pre.shape == (0, 5) and positions.shape == (15, 0, 2) and latents.shape == (15, 0, 4) and desc.shape == (0, 3) and not state.any()


def test_device_random_state_hands_the_call_on(monkeypatch):
    from spatiotemporal_variable_separation_amd.data.numpy_stream import DeviceRandomState
    rs = DeviceRandomState(np.random.RandomState(3), 'cpu')
    with pytest.raises(_lib.VarsepHipError, match='MI355X'):
        rs.stochastic_trajectories(3, 15, (0, 0, 0, -4, -4), (256, 37, 37, 5, 5), 36, 36, 4)
    seen = {}
    monkeypatch.setattr(ops, 'mmnist_stochastic_trajectories', lambda *a, **k: seen.update(a=a, k=k))
    rs.stochastic_trajectories(3, 15, (0,), (2,), 36, 35, 4, desc_nd=None, latents=True)
    assert seen['a'][0] is rs.state and seen['a'][1:] == (3, 15, (0,), (2,), 36, 35, 4) and seen['k'] == dict(validate=False, desc_nd=None, latents=True)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def test_cases_hold_what_the_walk_can_get_wrong():
    c = {x['name']: x for x in SI.cases()}
    r = SI.numpy_results()
    assert sorted(int(c['start_pos_%d' % p]['state'][N]) for p in SI.START_POSITIONS) == [0, 1, 227, 396, 397, 600, 623, 624]
    assert int(r['ends_on_624'][1][N]) == 624 and np.array_equal(r['ends_on_624'][1][:N], c['ends_on_624']['state'][:N])   # NumPy keeps the old key
    assert not np.array_equal(r['ends_on_624_then_goes_on'][1][:N], c['ends_on_624']['state'][:N])                          # and twists at the next draw
    assert [c[n]['calls'] for n in ('n0', 'n1', 'n6', 'n256')] == [[0], [1], [6], [256]] and all(c[n]['seq_len'] == 15 for n in ('n0', 'n1', 'n6', 'n256'))
    assert c['one_frame']['seq_len'] == 1
    assert c['tight_T100']['seq_len'] == 100 and c['tight_T100']['calls'] == [8]
    window = 4 * N
    assert int(c['tight_T100']['state'][N]) + sum(r['tight_T100'][2].outputs) > window           # past the first window
    assert max(r['tight_T400'][2].outputs) > window - N                                           # one trajectory that no window position holds
    assert sum(r['n256'][2].outputs) > window
    assert (c['tight_29']['frame'], c['tight_29']['digit'], c['tight_29']['max_speed']) == (29, (28, 28), 4)
    assert (c['tight_16_12_7']['frame'], c['tight_16_12_7']['digit'], c['tight_16_12_7']['max_speed']) == (16, (12, 12), 7)
    for n in ('rect_28x20', 'rect_12x30'):
        _, x_max, y_max = SI.geometry(c[n])
        assert x_max != y_max and min(x_max, y_max) >= 1
    assert c['max_speed_0']['max_speed'] == 0 and c['single_source_digit']['n_source'] == 1
    assert sum(r['max_speed_0'][2].outputs) > 0 and r['max_speed_0'][2].max_passes == 0          # only the start position consumes
    assert np.array_equal(r['n_pre_0_max_speed_0'][1], c['n_pre_0_max_speed_0']['state'])         # nothing consumes
    assert [c[n]['n_pre'] for n in ('n6', 'n_pre_4', 'n_pre_0_start_table')] == [5, 4, 0] and c['n_pre_0_start_table']['starts'][0].shape == (6, 4)
    assert c['split_3_3']['calls'] == [3, 3] and c['split_summed']['calls'] == [6]
    assert np.array_equal(c['split_3_3']['state'], c['split_summed']['state'])
    watches = [r[n][2] for n in r]
    assert any(w.redraws_across_blocks for w in watches) and any(w.prefixes_across_blocks for w in watches)
    assert any(w.max_passes >= 10 for w in watches) and max(w.max_passes for w in watches) < 64
    assert any(w.two_edge_passes for w in watches)
    # a trajectory straddles a regeneration in every case that starts near a block's end
    assert all(int(r['start_pos_%d' % p][1][N]) < p for p in (600, 623, 624))


def test_restatement_driven_by_numpy_equals_the_fixture():
    want, got = SI.golden_results(), SI.numpy_results()
    assert sorted(want) == sorted(got) == sorted(c['name'] for c in SI.cases())
    for name, (calls, words) in want.items():
        for (pre, traj), (my_pre, my_traj) in zip(calls, got[name][0]):
            assert np.array_equal(pre, my_pre) and np.array_equal(traj, my_traj), name
        assert np.array_equal(words, got[name][1]), name


# ---- the walk's logic on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """{lanes: {name: (statuses, calls, state words)}} of the host builds: 0 is the core's one-lane form, the others the lanes form."""
    tmp = tmp_path_factory.mktemp('mmnist_walk_host')
    plain, sanitized = SI.compile_host_check(tmp)
    lanes, lanes_sanitized = SI.compile_host_check(tmp, lanes=True)
    print('sanitizers: plain', sanitized, '| lanes', lanes_sanitized)
    out = {0: SI.run_host_check(plain, SI.cases(), tmp, lanes=1, tag='serial')}
    for n in (1,) + LANES:
        out[n] = SI.run_host_check(lanes, SI.cases(), tmp, lanes=n)
    return out


def _assert_equal(c, got, calls, words):
    statuses, got_calls, got_words = got
    assert statuses == [0] * len(c['calls']), (c['name'], statuses)
    for k, (g, (pre, traj)) in enumerate(zip(got_calls, calls)):
        positions, latents = SI.positions_of(traj)
        assert np.array_equal(g['pre'], pre), (c['name'], k, 'pre')
        assert np.array_equal(g['positions'], positions), (c['name'], k, 'positions')
        assert np.array_equal(g['latents'], latents), (c['name'], k, 'latents')
        if SI.desc_nd(c):
            assert np.array_equal(g['desc'], SI.desc_of(pre, SI.desc_nd(c))), (c['name'], k, 'desc')
    assert int(got_words[N]) == int(words[N]), (c['name'], 'pos')
    assert np.array_equal(got_words[:N], words[:N]), (c['name'], 'key')


@pytest.mark.parametrize('lanes', (0, 1) + LANES)
def test_core_on_the_host_equals_the_fixture_and_the_restatement_on_every_case(host, lanes):
    fixture, numpy = SI.golden_results(), SI.numpy_results()
    for c in SI.cases():
        _assert_equal(c, host[lanes][c['name']], *fixture[c['name']])
        _assert_equal(c, host[lanes][c['name']], *numpy[c['name']][:2])


def test_core_on_the_host_splits_like_one_call_and_keeps_the_old_key(host):
    for lanes in (0, 1) + LANES:
        got = host[lanes]
        for key in ('pre', 'positions', 'latents'):
            axis = 0 if key == 'pre' else 1
            assert np.array_equal(np.concatenate([call[key] for call in got['split_3_3'][1]], axis=axis), got['split_summed'][1][0][key])
        assert np.array_equal(got['split_3_3'][2], got['split_summed'][2])
        assert int(got['ends_on_624'][2][N]) == 624 and np.array_equal(got['ends_on_624'][2][:N], SI.case('ends_on_624')['state'][:N])
        assert np.array_equal(got['n_pre_0_max_speed_0'][2], SI.case('n_pre_0_max_speed_0')['state'])
        assert np.array_equal(got['n0'][2], SI.case('n0')['state'])


def test_core_on_the_host_refuses_a_position_past_the_block(tmp_path):
    bad = dict(SI.case('n6'), name='pos_625', state=start_state(9, 625))
    for lanes, count in ((False, 1), (True, 3)):
        exe, _ = SI.compile_host_check(tmp_path, lanes=lanes)
        statuses, calls, words = SI.run_host_check(exe, [bad], tmp_path, lanes=count, tag='bad')['pos_625']
        assert statuses == [1] and calls == [None] and np.array_equal(words, bad['state'])


# ---- the host route of the product ----------------------------------------------------------------------------------------------------
def _host_set(digits, frame, seq_len, max_speed, nd, monkeypatch):
    return MovingMNIST(digits, frame, 2, seq_len, max_speed, False, nd, True, device='cpu')


@pytest.mark.parametrize('name', ['n6', 'n256', 'tight_29', 'rect_28x20', 'single_source_digit', 'max_speed_0', 'split_3_3'])
def test_host_route_of_draw_stochastic_equals_the_fixture_and_leaves_the_stream_where_numpys_is(name, monkeypatch):
    c = SI.case(name)
    calls, words = SI.golden_results()[name]
    ds = _host_set(np.zeros((c['n_source'],) + c['digit'], dtype=np.uint8), c['frame'], c['seq_len'], c['max_speed'], 2, monkeypatch)
    ds.rng = random_state_at(c['state'])
    global_before = np.random.get_state()
    for n, (pre, traj) in zip(c['calls'], calls):
        if n % 2:                                                              # three trajectories: videos of one digit
            ds.num_digits = 1
        nd = ds.num_digits
        desc, positions = ds.draw_stochastic(n // nd)
        assert desc.dtype == positions.dtype == np.int32 and positions.shape == (c['seq_len'], n // nd, nd, 2)
        assert np.array_equal(desc, SI.desc_of(pre, nd)) and np.array_equal(positions.reshape(c['seq_len'], n, 2), SI.positions_of(traj)[0])
    assert np.array_equal(state_words(ds.rng), words)
    assert np.array_equal(np.random.get_state()[1], global_before[1]) and np.random.get_state()[2] == global_before[2]


def test_host_route_draws_from_the_global_stream_when_no_private_one_is_set(monkeypatch):
    c = SI.case('n6')
    (pre, traj), = SI.golden_results()['n6'][0]
    ds = _host_set(np.zeros((256, 28, 28), dtype=np.uint8), 64, 15, 4, 2, monkeypatch)
    kept = np.random.get_state()
    try:
        np.random.set_state(random_state_at(c['state']).get_state())
        desc, positions = ds.draw_stochastic(3)
        assert np.array_equal(state_words(np.random), SI.golden_results()['n6'][1])
    finally:
        np.random.set_state(kept)
    assert np.array_equal(desc, SI.desc_of(pre, 2)) and np.array_equal(positions.reshape(15, 6, 2), SI.positions_of(traj)[0])


def test_stochastic_set_constructs_and_refuses_a_digit_that_fills_the_frame(monkeypatch):
    blobs = mmnist_ref.blobs()
    ds = _host_set(blobs, 64, 6, 4, 2, monkeypatch)
    assert ds.deterministic is False and ds.train and ds.digit_shape == (28, 28) and len(ds) == 200000
    with pytest.raises(ValueError, match='fills the 28 x 28 frame'):
        _host_set(blobs, 28, 6, 4, 2, monkeypatch)
    MovingMNIST(blobs, 28, 2, 6, 4, True, 2, True, device='cpu')              # the deterministic set takes it, as before
    assert 'NotImplementedError' not in open(moving_mnist.__file__).read()


# ---- the flag ---------------------------------------------------------------------------------------------------------------------------
def test_flag_parses_and_main_constructs_the_stochastic_set(monkeypatch):
    base = ['--xp_dir', 'x', '--data_dir', 'synthetic_digits', '--data', 'mnist']
    assert options.parser.parse_args(base).mnist_stochastic is False
    assert options.parser.parse_args(base + ['--mnist_stochastic']).mnist_stochastic is True
    seen = []
    monkeypatch.setattr(MovingMNIST, 'make_dataset', classmethod(lambda cls, *a, **k: seen.append((a, k)) or 'set'))
    for flag in ([], ['--mnist_stochastic']):
        args = options.parser.parse_args(base + flag + ['--n_object', '3', '--nt_cond', '2', '--nt_pred', '4'])
        assert vs_main.load_dataset(args, torch.device('cuda', 0)) == 'set'
    (a0, k0), (a1, k1) = seen
    assert a0 == ('synthetic_digits', 64, 2, 6, 4, True, 3, True) and a1 == ('synthetic_digits', 64, 2, 6, 4, False, 3, True)
    assert k0 == k1 and set(k0) == {'device', 'seed'}

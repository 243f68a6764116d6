"""GPU: vs_mmnist_stochastic_trajectories (csrc/vs_mmnist_walk.hip) through ops.mmnist_stochastic_trajectories on the cases of
tests/smnist_inputs.py -- prefix draws, positions, latents, desc and the downloaded state bit-equal to the fixture written from the
reference's own sampler (tests/golden/smnist.npz), with guard bytes round every output and the state --, the stochastic MovingMNIST set
against the reference's frames, the host route against the device route, and `main --mnist_stochastic` with VARSEP_MMNIST_DRAWS=device."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import smnist_inputs as SI
from guard_util import embed, guarded_ops
from golden_util import load_golden
from mmnist_draws_inputs import N, ROOT, random_state_at, start_state, state_words
from oracle import mmnist_ref
from spatiotemporal_variable_separation_amd import _lib, ops
from spatiotemporal_variable_separation_amd.data.moving_mnist import MovingMNIST
from spatiotemporal_variable_separation_amd.data.numpy_stream import DeviceRandomState

pytestmark = pytest.mark.gpu
NAMES = [c['name'] for c in SI.cases()]


def _upload(words):
    """The state on the device, between two bands of guard bytes."""
    return embed(torch.from_numpy(np.asarray(words, dtype=np.uint32).view(np.int32).copy()).cuda())


def _walk(c, state, k, **kwargs):
    cols, x_max, y_max = SI.geometry(c)
    start = torch.from_numpy(c['starts'][k]).cuda() if c['starts'] else None
    return ops.mmnist_stochastic_trajectories(state, c['calls'][k], c['seq_len'], [a for a, _ in cols], [b for _, b in cols], x_max, y_max,
                                              c['max_speed'], start=start, latents=True, desc_nd=SI.desc_nd(c) or None, **kwargs)


@pytest.fixture(scope='module')
def walked():
    """{name: (calls, state words)}: every case through the op, once; every output the op allocates and the state lie between guard bytes."""
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        allocs = guarded_ops(mp)
        for c in SI.cases():
            state, state_guard = _upload(c['state'])
            calls = []
            for k in range(len(c['calls'])):
                pre, positions, latents, desc = _walk(c, state, k)
                calls.append(dict(pre=pre.cpu().numpy(), positions=positions.cpu().numpy(), latents=latents.cpu().numpy(),
                                  desc=None if desc is None else desc.cpu().numpy()))
            state_guard.check()
            out[c['name']] = (calls, state.cpu().numpy().view(np.uint32))
        allocs.check()                                                      # a store outside [seq_len, n_traj, *] of any output shows here
        assert len(allocs.guards) >= 4 * sum(len(c['calls']) for c in SI.cases() if SI.desc_nd(c))
    return out


@pytest.mark.parametrize('name', NAMES)
def test_kernel_equals_the_fixture(name, walked):
    c = SI.case(name)
    calls, words = walked[name]
    ref_calls, ref_words = SI.golden_results()[name]
    for k, (got, (pre, traj)) in enumerate(zip(calls, ref_calls)):
        positions, latents = SI.positions_of(traj)
        assert got['pre'].dtype == np.int32 and got['pre'].shape == pre.shape and np.array_equal(got['pre'], pre), (k, 'pre')
        assert got['positions'].shape == positions.shape and np.array_equal(got['positions'], positions), (k, 'positions')
        assert got['latents'].shape == latents.shape and np.array_equal(got['latents'], latents), (k, 'latents')
        if SI.desc_nd(c):
            assert np.array_equal(got['desc'], SI.desc_of(pre, SI.desc_nd(c))), (k, 'desc')
    assert int(words[N]) == int(ref_words[N]), 'pos'
    assert np.array_equal(words[:N], ref_words[:N]), 'key'


def test_split_launches_equal_one_and_the_outputs_agree_among_themselves(walked):
    split, whole = walked['split_3_3'], walked['split_summed']
    for key, axis in (('pre', 0), ('positions', 1), ('latents', 1)):
        assert np.array_equal(np.concatenate([call[key] for call in split[0]], axis=axis), whole[0][0][key]), key
    assert np.array_equal(split[1], whole[1])
    for name, (calls, _) in walked.items():
        c = SI.case(name)
        for call in calls:
            assert np.array_equal(call['latents'][:, :, :2], call['positions']), name
            if c['n_pre'] >= 4 and call['pre'].shape[0]:
                assert np.array_equal(call['latents'][0, :, :2], call['pre'][:, -4:-2]), name      # no bounce before the first frame
            if call['desc'] is not None:
                assert np.array_equal(call['desc'], SI.desc_of(call['pre'], 2)), name
    assert int(walked['ends_on_624'][1][N]) == 624
    assert np.array_equal(walked['ends_on_624'][1][:N], SI.case('ends_on_624')['state'][:N])                 # the old key came back
    assert np.array_equal(walked['n_pre_0_max_speed_0'][1], SI.case('n_pre_0_max_speed_0')['state'])         # nothing was consumed


def test_kernel_equals_the_host_build(walked, tmp_path):
    exe, _ = SI.compile_host_check(tmp_path)
    host = SI.run_host_check(exe, SI.cases(), tmp_path)
    for c in SI.cases():
        statuses, calls, words = host[c['name']]
        got_calls, got_words = walked[c['name']]
        assert statuses == [0] * len(c['calls'])
        for got, want in zip(got_calls, calls):
            assert all(np.array_equal(got[key], want[key]) for key in ('pre', 'positions', 'latents')), c['name']
        assert np.array_equal(got_words, words), c['name']


def test_a_position_past_the_block_raises_and_touches_nothing(monkeypatch):
    c = SI.case('n6')
    words = start_state(9, 625)
    state, state_guard = _upload(words)
    with pytest.raises(_lib.VarsepHipError, match='pos above 624'):
        _walk(c, state, 0)
    allocs = guarded_ops(monkeypatch)
    pre, positions, latents, desc = _walk(c, state, 0, validate=False)      # unvalidated: the same refusal, silently
    allocs.check()
    state_guard.check()
    for t in (pre, positions, latents, desc):
        assert bool((t == -1).all())                                        # the prefill (0xFF bytes) is still there
    assert np.array_equal(state.cpu().numpy().view(np.uint32), words)


@pytest.mark.parametrize('key,frame,seed', SI.FRAME_SETS)
def test_stochastic_set_on_a_device_stream_gives_the_reference_frames(key, frame, seed):
    g = SI.golden()
    want = torch.from_numpy(g[key + ':u8'].astype(np.float32) / 255).cuda()                 # [3, 6, 1, F, F]
    for dtype in (torch.float32, torch.bfloat16):
        ds = MovingMNIST(mmnist_ref.blobs(), frame, SI.FRAME_COND, SI.FRAME_LEN, 4, False, SI.FRAME_DIGITS, True, device='cuda')
        ds.rng = DeviceRandomState(random_state_at(g[key + ':state']), 'cuda')
        cond, target = ds.batch(SI.FRAME_ITEMS, dtype)
        assert cond.dtype == dtype and cond.shape == (3, SI.FRAME_COND, 1, frame, frame) and target.shape == (3, SI.FRAME_LEN - SI.FRAME_COND, 1, frame, frame)
        assert torch.equal(torch.cat([cond, target], dim=1), want.to(dtype)), dtype        # bit for bit; bf16: the rounded fixture
        assert np.array_equal(state_words(ds.rng.to_random_state()), g[key + ':final'])
    one = MovingMNIST(mmnist_ref.blobs(), frame, SI.FRAME_COND, SI.FRAME_LEN, 4, False, SI.FRAME_DIGITS, True, device='cuda')
    one.rng = DeviceRandomState(random_state_at(g[key + ':state']), 'cuda')
    cond, target = one[0]                                                                   # __getitem__: one item
    assert torch.equal(torch.cat([cond, target]), want[0])


def _digits(shape):
    blobs = mmnist_ref.blobs(n=20, seed=5)
    h, w = shape
    return np.ascontiguousarray(np.pad(blobs, ((0, 0), ((h - 28) // 2, h - 28 - (h - 28) // 2), ((w - 28) // 2, w - 28 - (w - 28) // 2))))


@pytest.mark.parametrize('frame,nd,shape,speed', [(64, 2, (28, 28), 4), (64, 3, (28, 28), 4), (32, 1, (28, 28), 4), (40, 2, (30, 28), 7)])
def test_host_and_device_routes_give_equal_batches_from_equal_seeds(frame, nd, shape, speed):
    """Three consecutive batch(8) calls on each route."""
    digits, seed = _digits(shape), 2000 + frame + nd
    on_host = MovingMNIST(digits, frame, 2, 6, speed, False, nd, True, device='cuda')
    on_device = MovingMNIST(digits, frame, 2, 6, speed, False, nd, True, device='cuda')
    on_host.rng = np.random.RandomState(seed)
    on_device.rng = DeviceRandomState(np.random.RandomState(seed), 'cuda')
    desc, positions = on_device.draw_stochastic(8)
    assert desc.is_cuda and desc.dtype == positions.dtype == torch.int32 and desc.shape == (8, 1 + nd) and positions.shape == (6, 8, nd, 2)
    on_device.rng = DeviceRandomState(np.random.RandomState(seed), 'cuda')
    global_before = np.random.get_state()
    for call in range(3):
        want_cond, want_target = on_host.batch(8)
        cond, target = on_device.batch(8)
        assert cond.shape == want_cond.shape == (8, 2, 1, frame, frame) and target.shape == want_target.shape == (8, 4, 1, frame, frame)
        assert torch.equal(cond, want_cond) and torch.equal(target, want_target), call
        assert float(cond.max()) > 0
    assert np.array_equal(state_words(on_device.rng.to_random_state()), state_words(on_host.rng))
    assert np.array_equal(np.random.get_state()[1], global_before[1]) and np.random.get_state()[2] == global_before[2]


def test_a_deterministic_batch_drawn_beside_a_stochastic_one_equals_todays():
    z = load_golden('moving_mnist')
    frame, nt_cond, seq_len, max_speed, nd, batch, seed = [int(v) for v in z['default:params']]
    want = torch.from_numpy(z['default:frames_u8'].astype(np.float32) / 255).cuda()
    det = MovingMNIST(z['digits'], frame, nt_cond, seq_len, max_speed, True, nd, True, device='cuda')
    sto = MovingMNIST(z['digits'], frame, nt_cond, seq_len, max_speed, False, nd, True, device='cuda')
    det.rng = DeviceRandomState(np.random.RandomState(seed), 'cuda')        # np.random.seed(seed) of the fixture is RandomState(seed)
    sto.rng = DeviceRandomState(np.random.RandomState(seed + 1), 'cuda')
    sto.batch(4)
    cond, target = det.batch(batch)
    sto.batch(4)
    assert torch.equal(torch.cat([cond, target], dim=1), want)
    host = np.random.RandomState(seed)                                      # and the host route beside it
    det_host = MovingMNIST(z['digits'], frame, nt_cond, seq_len, max_speed, True, nd, True, device='cuda')
    det_host.rng = host
    cond_h, target_h = det_host.batch(batch)
    assert torch.equal(cond_h, cond) and torch.equal(target_h, target)
    assert np.array_equal(state_words(det.rng.to_random_state()), state_words(host))


def test_main_trains_on_the_stochastic_set_with_the_draws_on_the_device(tmp_path):
    cmd = [sys.executable, '-m', 'spatiotemporal_variable_separation_amd.main', '--xp_dir', str(tmp_path), '--data_dir', 'synthetic_digits',
           '--data', 'mnist', '--mnist_stochastic', '--device', '0', '--epochs', '1', '--batch_size', '8', '--num_workers', '0', '--seed', '3',
           '--log_interval', '1', '--nt_cond', '2', '--nt_pred', '3', '--offset', '2', '--enc_hidden_size', '8', '--dec_hidden_size', '8',
           '--res_hidden_size', '16', '--code_size_s', '12', '--code_size_t', '6', '--precision', 'bf16', '--hip_graph']
    env = dict(os.environ, VARSEP_MMNIST_EPOCH_LEN='16', VARSEP_MMNIST_DRAWS='device')
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    losses = [float(v) for v in re.findall(r'step \d+: total (\S+)', r.stdout)]
    assert len(losses) == 2 and all(np.isfinite(losses)), r.stdout[-2000:]
    assert 'frames/s' in r.stdout and (tmp_path / 'decoder.pt').exists()

"""GPU: vs_mt19937_randint (csrc/vs_mt19937.hip) through ops.mt19937_randint on the cases of tests/mmnist_draws_inputs.py -- tables and the
downloaded state bit-equal to NumPy's and to the host build's, with guard bytes round the table and the state --, DeviceRandomState, the
Moving-MNIST training batches drawn on the device against the same batches drawn on the host, and `main` with VARSEP_MMNIST_DRAWS=device."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mmnist_draws_inputs as MD
from guard_util import embed, window
from oracle import mmnist_ref
from spatiotemporal_variable_separation_amd import _lib, ops
from spatiotemporal_variable_separation_amd.data.moving_mnist import MovingMNIST
from spatiotemporal_variable_separation_amd.data.numpy_stream import DeviceRandomState

pytestmark = pytest.mark.gpu
ROOT = MD.ROOT
NAMES = [c['name'] for c in MD.cases()]


def _upload(words):
    """The state on the device, between two bands of guard bytes."""
    return embed(torch.from_numpy(np.asarray(words, dtype=np.uint32).view(np.int32).copy()).cuda())


@pytest.fixture(scope='module')
def drawn():
    """{name: (tables, state words)}: every case through ops.mt19937_randint, once; tables and state lie between guard bytes."""
    out = {}
    for c in MD.cases():
        state, state_guard = _upload(c['state'])
        lows, highs = [a for a, _ in c['cols']], [b for _, b in c['cols']]
        tables = []
        for rows in c['calls']:
            if rows == 0:
                tables.append(ops.mt19937_randint(state, lows, highs, 0).cpu().numpy())
                continue
            table, guard = window((rows, len(lows)), torch.int32, device='cuda')
            got = ops.mt19937_randint(state, lows, highs, rows, out=table)
            assert got is table
            guard.check()
            tables.append(table.cpu().numpy())
        state_guard.check()
        out[c['name']] = (tables, state.cpu().numpy().view(np.uint32))
    return out


@pytest.mark.parametrize('name', NAMES)
def test_kernel_equals_numpy(name, drawn):
    tables, words = drawn[name]
    ref_tables, ref_words = MD.numpy_results()[name]
    for call, (got, ref) in enumerate(zip(tables, ref_tables)):
        assert got.dtype == np.int32 and got.shape == ref.shape and np.array_equal(got, ref), (name, call)
    assert int(words[MD.N]) == int(ref_words[MD.N]), 'pos'
    assert np.array_equal(words[:MD.N], ref_words[:MD.N]), 'key'


def test_kernel_equals_the_host_build(drawn, tmp_path):
    exe, _ = MD.compile_host_check(tmp_path)
    host = MD.run_host_check(exe, MD.cases(), tmp_path)
    for c in MD.cases():
        statuses, tables, words = host[c['name']]
        got_tables, got_words = drawn[c['name']]
        assert statuses == [0] * len(c['calls'])
        assert all(np.array_equal(a, b) for a, b in zip(got_tables, tables)) and np.array_equal(got_words, words), c['name']


def test_kernel_consumes_nothing_for_zero_ranges_and_splits_like_one_call(drawn):
    assert np.array_equal(drawn['rng0_every_column'][1], MD.case('rng0_every_column')['state'])
    assert np.array_equal(drawn['rng0_every_column'][0][0], np.tile([5, 0, -3], (9, 1)))
    assert np.array_equal(np.concatenate(drawn['back_to_back'][0]), drawn['back_to_back_summed'][0][0])
    assert np.array_equal(drawn['back_to_back'][1], drawn['back_to_back_summed'][1])
    assert int(drawn['ends_on_624'][1][MD.N]) == 624
    assert np.array_equal(drawn['ends_on_624'][1][:MD.N], MD.case('ends_on_624')['state'][:MD.N])            # the old key came back


def test_a_position_past_the_block_raises_and_touches_nothing():
    words = MD.start_state(9, 625)
    state, state_guard = _upload(words)
    table, guard = window((4, 5), torch.int32, device='cuda')
    lows, highs = zip(*MD.product_cols())
    with pytest.raises(_lib.VarsepHipError, match='pos above 624'):
        ops.mt19937_randint(state, lows, highs, 4, out=table)
    guard.check()
    state_guard.check()
    assert bool((table == -1).all())                                        # the prefill (0xFF bytes) is still there
    assert np.array_equal(state.cpu().numpy().view(np.uint32), words)
    ops.mt19937_randint(state, lows, highs, 4, out=table, validate=False)   # unvalidated: the same refusal, silently
    assert bool((table == -1).all()) and np.array_equal(state.cpu().numpy().view(np.uint32), words)

    class Source:
        @staticmethod
        def get_state():
            return ('MT19937', words[:MD.N], 625, 0, 0.0)

    with pytest.raises(_lib.VarsepHipError, match='pos 625'):               # and DeviceRandomState never uploads such a state
        DeviceRandomState(Source, 'cuda')


def test_two_device_streams_used_alternately_stay_independent():
    lows, highs = zip(*MD.product_cols())
    a, b = DeviceRandomState(np.random.RandomState(1), 'cuda'), DeviceRandomState(np.random.RandomState(2), 'cuda')
    ha, hb = np.random.RandomState(1), np.random.RandomState(2)
    for rows in (3, 70, 1, 200):
        ta, tb = a.randint_table(lows, highs, rows), b.randint_table(lows, highs, rows)
        for got, host in ((ta, ha), (tb, hb)):
            want = np.array([[host.randint(lo, hi) for lo, hi in zip(lows, highs)] for _ in range(rows)])
            assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    for dev, host in ((a, ha), (b, hb)):
        assert np.array_equal(MD.state_words(dev.to_random_state()), MD.state_words(host))


def test_get_state_leaves_the_stream_where_it_was_and_keeps_the_gaussian_cache():
    source = np.random.RandomState(77)
    source.standard_normal(3)                                               # a Gaussian is cached
    global_before = np.random.get_state()
    dev = DeviceRandomState(source, 'cuda')
    first = dev.randint_table([0, -4], [37, 5], 50).cpu().numpy()
    s1, s2 = dev.get_state(), dev.get_state()
    assert s1[0] == 'MT19937' and s1[2] == s2[2] and np.array_equal(s1[1], s2[1]) and s1[3:] == source.get_state()[3:] and s1[3] == 1
    second = dev.randint_table([0, -4], [37, 5], 50).cpu().numpy()
    want = np.array([[source.randint(0, 37), source.randint(-4, 5)] for _ in range(100)])
    assert np.array_equal(np.concatenate([first, second]), want)
    host = dev.to_random_state()
    assert host.standard_normal() == source.standard_normal() and host.randint(0, 1000) == source.randint(0, 1000)
    snapshot = DeviceRandomState(None, 'cuda')                              # the global stream: copied, not advanced
    after = np.random.get_state()
    assert after[2] == global_before[2] and np.array_equal(after[1], global_before[1])
    assert np.array_equal(snapshot.get_state()[1], global_before[1]) and snapshot.get_state()[2] == global_before[2]


def _digits(shape):
    blobs = mmnist_ref.blobs(n=20, seed=5)
    h, w = shape
    return np.ascontiguousarray(np.pad(blobs, ((0, 0), ((h - 28) // 2, h - 28 - (h - 28) // 2), ((w - 28) // 2, w - 28 - (w - 28) // 2))))


@pytest.mark.parametrize('frame,nd,shape', [(64, 1, (28, 28)), (64, 3, (28, 28)), (40, 1, (28, 28)), (40, 3, (28, 28)), (40, 2, (40, 28))])
def test_batches_drawn_on_the_device_equal_the_batches_drawn_on_the_host(frame, nd, shape):
    """Three consecutive batch(8) calls; the last parameter set has frame == digit height: the start-row column has rng == 0."""
    digits, seed = _digits(shape), 1000 + frame + nd
    on_host = MovingMNIST(digits, frame, 2, 6, 4, True, nd, True, device='cuda')
    on_device = MovingMNIST(digits, frame, 2, 6, 4, True, nd, True, device='cuda')
    on_host.rng = np.random.RandomState(seed)
    on_device.rng = DeviceRandomState(np.random.RandomState(seed), 'cuda')
    global_before = np.random.get_state()
    for _ in range(3):
        init = on_device.draw(8)
        assert init.is_cuda and init.dtype == torch.int32 and init.shape == (8, nd, 5)
    on_device.rng = DeviceRandomState(np.random.RandomState(seed), 'cuda')
    for call in range(3):
        want_cond, want_target = on_host.batch(8)
        cond, target = on_device.batch(8)
        assert cond.shape == want_cond.shape == (8, 2, 1, frame, frame) and target.shape == want_target.shape == (8, 4, 1, frame, frame)
        assert torch.equal(cond, want_cond) and torch.equal(target, want_target), call
        assert float(cond.max()) > 0
    assert np.array_equal(MD.state_words(on_device.rng.to_random_state()), MD.state_words(on_host.rng))
    assert np.array_equal(np.random.get_state()[1], global_before[1]) and np.random.get_state()[2] == global_before[2]


def test_main_trains_with_the_draws_on_the_device(tmp_path):
    cmd = [sys.executable, '-m', 'spatiotemporal_variable_separation_amd.main', '--xp_dir', str(tmp_path), '--data_dir', 'synthetic_digits',
           '--data', 'mnist', '--device', '0', '--epochs', '1', '--batch_size', '8', '--num_workers', '0', '--seed', '3', '--log_interval', '1',
           '--nt_cond', '2', '--nt_pred', '3', '--offset', '2', '--enc_hidden_size', '8', '--dec_hidden_size', '8', '--res_hidden_size', '16',
           '--code_size_s', '12', '--code_size_t', '6', '--precision', 'bf16', '--hip_graph']
    env = dict(os.environ, VARSEP_MMNIST_EPOCH_LEN='32', VARSEP_MMNIST_DRAWS='device')
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'frames/s' in r.stdout and (tmp_path / 'decoder.pt').exists()

"""GPU: the WaveEq simulation kernel (vs_wave_simulate) against the fp64 NumPy reference of tests/wave_sim_ref.py, the files gen_wave writes
against the set simulated straight into HBM, and training on `--data_dir simulated`.

Tolerance of the comparisons with fp64: the yardstick is the max-abs error of the fp32 run of the SAME NumPy reference against its fp64 run on the
same inputs, computed here on every run; the kernel may be at most 4x that far from fp64.  The system is linear, so rounding error grows gently;
FMA contraction and the compiler's freedom in the stencil account for a small factor and no more.
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import wave_sim_ref as R
from oracle import wave_data_ref
from spatiotemporal_variable_separation_amd import ops
from spatiotemporal_variable_separation_amd.data.wave_eq import WaveEq, WaveEqPartial
from spatiotemporal_variable_separation_amd.preprocessing.wave import gen_pixels, gen_wave

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(30.0, 400.0), (1.0, 300.0), (17.3, 351.7)]
BOUND = 4.0


def report(what, got, ref64, ref32):
    yard = np.abs(ref32.astype(np.float64) - ref64).max()
    err = np.abs(got.astype(np.float64) - ref64).max()
    print('%s: amplitude %.3g, fp32 NumPy vs fp64 %.3g, kernel vs fp64 %.3g, ratio %.2f' % (what, np.abs(ref64).max(), yard, err, err / yard))
    return err, yard


def test_border_rule_from_a_random_start():
    """3 sequences, 6 frames, randn start: every frame against fp64.  O(1) magnitudes: a wrong border band, a swapped axis, a wrong tableau
    coefficient or a source-table index slip is orders of magnitude above rounding.  Measured on the MI355X: kernel vs fp64 6.1e-7 on an amplitude
    of 4.2, against a yardstick of 8.6e-7: ratio 0.71."""
    f0, c = zip(*PAIRS)
    init = torch.randn((3, 2, 64, 64), generator=torch.Generator().manual_seed(11))
    got, minmax = ops.wave_simulate(f0, c, 6, init=init.cuda())
    ref64 = R.simulate_many(f0, c, 6, init=init.numpy(), dtype=np.float64)
    ref32 = R.simulate_many(f0, c, 6, init=init.numpy(), dtype=np.float32)
    assert np.abs(ref64[:, -1, :2]).max() > 0.1                     # the border cells do move from this start
    got = got.cpu().numpy()
    assert np.array_equal(got[:, 0], init[:, 0].numpy())
    err, yard = report('random start, T = 6', got, ref64, ref32)
    assert err <= BOUND * yard
    assert np.array_equal(minmax.cpu().numpy(), np.stack([got.reshape(3, -1).min(1), got.reshape(3, -1).max(1)], axis=1))


@pytest.fixture(scope='module')
def real_regime():
    rng = np.random.RandomState(5)
    pairs = PAIRS + [(rng.uniform(1, 30), rng.uniform(300, 400)) for _ in range(2)]
    f0, c = zip(*pairs)
    got, minmax = ops.wave_simulate(f0, c, 300)
    return f0, c, got, minmax, R.simulate_many(f0, c, 300, dtype=np.float64), R.simulate_many(f0, c, 300, dtype=np.float32)


def test_real_regime_against_fp64(real_regime):
    """Zero start, 5 sequences, 300 frames, per sequence (amplitudes differ 30-fold with f0).  Measured on the MI355X, kernel vs fp64 over the
    yardstick: 1.00, 0.99, 0.99, 0.99, 0.99 for the five sequences (1.94e-7 against 1.95e-7 on an amplitude of 3.2e-3 at f0 = 30, c = 400)."""
    f0, c, got, minmax, ref64, ref32 = real_regime
    got, minmax = got.cpu().numpy(), minmax.cpu().numpy()
    assert got.shape == (5, 300, 64, 64) and got.dtype == np.float32
    for k in range(5):
        err, yard = report('zero start, T = 300, f0 = %.4g, c = %.4g' % (f0[k], c[k]), got[k], ref64[k], ref32[k])
        assert err <= BOUND * yard
        assert abs(minmax[k, 0] - ref64[k].min()) <= BOUND * yard and abs(minmax[k, 1] - ref64[k].max()) <= BOUND * yard
        assert minmax[k, 0] == got[k].min() and minmax[k, 1] == got[k].max()
    assert np.all(got[:, 0] == 0)
    for band in (got[:, :, [0, 1, 62, 63], :], got[:, :, :, [0, 1, 62, 63]]):
        assert np.all(band == 0)


def test_sequences_do_not_depend_on_their_launch(real_regime):
    f0, c, got, minmax = real_regime[:4]
    for k in (0, 3):
        alone, mm = ops.wave_simulate([f0[k]], [c[k]], 300)
        assert torch.equal(alone[0], got[k]) and torch.equal(mm[0], minmax[k])


def test_normalised_output_is_the_loaders_arithmetic(real_regime):
    f0, c, got = real_regime[:3]
    norm, minmax = ops.wave_simulate(f0[:2], c[:2], 300, normalise=True)
    for k in range(2):
        x = got[k].cpu()
        assert torch.equal(norm[k].cpu(), (x - x.min()) / (x.max() - x.min()))      # data/wave_eq.py, on the host
        assert minmax[k, 0].item() == x.min().item() and minmax[k, 1].item() == x.max().item()


@pytest.fixture(scope='module')
def generated_dir():
    d = wave_data_ref.fixture_dir() + '_generated'
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d)
    gen_wave.main(['--data_dir', d, '--device', '0', '--size', '10', '--seq_len', '12', '--seed', '3'])
    gen_pixels.main(['--data_dir', d, '--number', '9'])
    yield d
    shutil.rmtree(d, ignore_errors=True)


def test_generated_files_have_the_reference_format(generated_dir):
    f0, c = gen_wave.wave_parameters(10, 3)
    assert sorted(os.listdir(os.path.join(generated_dir, 'data'))) == sorted('homogenous_wave%d.pt' % i for i in range(10))
    for i in (0, 9):
        d = torch.load(os.path.join(generated_dir, 'data', 'homogenous_wave%d.pt' % i))
        assert sorted(d) == ['c', 'simul'] and type(d['c']) is float and d['c'] == c[i]
        assert d['simul'].device.type == 'cpu' and d['simul'].dtype == torch.float32 and tuple(d['simul'].shape) == (12, 64, 64)
    direct, _ = ops.wave_simulate(f0[9:], c[9:], 12)
    assert torch.equal(direct[0].cpu(), d['simul'])


@pytest.mark.parametrize('train', [True, False])
def test_files_and_hbm_route_agree(generated_dir, train):
    with wave_data_ref.sorted_listdir():
        from_files = WaveEq(generated_dir, 2, 5, train, 1)
        part_files = WaveEqPartial(generated_dir, 2, 5, train, 1, 7)
    in_hbm = WaveEq.simulated(2, 5, train, 1, size=10, sim_len=12, seed=3)
    part_hbm = WaveEqPartial.simulated(2, 5, train, 1, 7, size=10, sim_len=12, seed=3, n_drawn=9)
    n = (8 if train else 2)
    assert from_files.size == in_hbm.size == n and len(from_files) == len(in_hbm) and in_hbm.nt == 12 and in_hbm.frame_shape == (64, 64)
    assert np.array_equal(in_hbm.velocities, gen_wave.wave_parameters(10, 3)[1][:8] if train else gen_wave.wave_parameters(10, 3)[1][8:])
    assert torch.equal(from_files.all_data, in_hbm.all_data)        # the same sequences in the same order, normalised to the same bits
    items = list(range(n * 8))                                      # every window: 12 + 1 - 5 per sequence
    for a, b in ((from_files, in_hbm), (part_files, part_hbm)):
        for x, y in zip(a.batch(items), b.batch(items)):
            assert x.shape == y.shape and torch.equal(x, y)
    assert part_hbm.batch(items)[0].shape == (n * 8, 2, 1, 7)
    assert np.array_equal(part_files.rand_w, part_hbm.rand_w) and np.array_equal(part_files.rand_h, part_hbm.rand_h)
    down = WaveEq.simulated(2, 3, train, 2, size=10, sim_len=12, seed=3)
    assert torch.equal(down.all_data, in_hbm.all_data.view(n, 12, -1)[:, ::2])


DRIVER = '''
import sys
from spatiotemporal_variable_separation_amd.data.wave_eq import WaveEq
full = WaveEq.simulated.__func__
WaveEq.simulated = classmethod(lambda cls, *a, **k: full(cls, *a, size=5, sim_len=64, **k))   # 4 training sequences of 64 frames
from spatiotemporal_variable_separation_amd.main import main
main(sys.argv[1:])
'''


def test_main_trains_on_the_simulated_set(tmp_path):
    """`main --data wave --data_dir simulated`, the flags of tests/test_main_gpu.py for wave.  main has no flag that sizes the simulated set, so
    the child process shrinks the defaults of `WaveEq.simulated` (64 frames: as many as rows, so that the reference's `__len__` quirk stays
    inside the set): 4 x 58 windows in batches of 116 are two steps."""
    cmd = [sys.executable, '-c', DRIVER, '--xp_dir', str(tmp_path), '--data_dir', 'simulated', '--device', '0', '--epochs', '1',
           '--batch_size', '116', '--num_workers', '0', '--seed', '3', '--log_interval', '1', '--chkpt_interval', '1', '--downsample', '1',
           '--data', 'wave', '--architecture', 'mlp', '--nt_cond', '3', '--nt_pred', '4', '--offset', '3', '--code_size_t', '8',
           '--code_size_s', '8', '--mixing', 'mul', '--enc_hidden_size', '64', '--dec_hidden_size', '64', '--res_hidden_size', '32',
           '--n_blocks', '2']
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    totals = [float(line.split('total')[1].split()[0]) for line in r.stdout.splitlines() if line.startswith('epoch') and 'total' in line]
    assert len(totals) == 2 and all(np.isfinite(totals)), r.stdout[-2000:]


def test_load_dataset_builds_the_papers_set():
    from spatiotemporal_variable_separation_amd.main import load_dataset
    from spatiotemporal_variable_separation_amd.options import parser
    args = parser.parse_args(['--xp_dir', 'x', '--data_dir', 'simulated', '--data', 'wave_partial', '--nt_cond', '5', '--nt_pred', '20'])
    ds = load_dataset(args, torch.device('cuda', 0))
    assert isinstance(ds, WaveEqPartial) and ds.size == 240 and ds.nt == 150 and ds._pixels.numel() == 100
    x = ds.all_data
    assert x.min().item() == 0.0 and x.max().item() == 1.0 and torch.isfinite(x).all()
    cond, target = ds.batch([0, len(ds) - 1])
    assert cond.shape == (2, 5, 1, 100) and target.shape == (2, 20, 1, 100)

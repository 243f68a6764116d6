"""GPU: the evaluation CLIs (spatiotemporal_variable_separation_amd.test.mnist.test / .test_disentanglement / .test.wave.test) against
the reference's own outputs on the same inputs (tests/golden/eval_cli_*, written by tests/make_golden_eval_cli.py), and their kernels
(csrc/vs_eval.hip): vs_moving_mnist_place, vs_frame_metrics_multi, vs_frames_to_u8_nhwc."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import eval_cli_inputs as I
from cli_util import close, run_module
from golden_util import GOLDEN_DIR
from oracle.wave_data_ref import fixture_dir, sorted_listdir

pytestmark = pytest.mark.gpu

DATA_ARRAYS = {'gt.npz', 'cond.npz', 'cond_swap.npz', 'target_swap.npz', 'content_swap_gt.npz', 'cond_swap_test.npz', 'target_swap_test.npz'}
MODEL_ARRAYS = {'predictions.npz', 'content_swap.npz', 'content_swap_test.npz'}
OUTPUTS = {'test': ['results.npz', 'predictions.npz', 'gt.npz', 'cond.npz', 'content_swap.npz', 'cond_swap.npz', 'target_swap.npz'],
           'test_disentanglement': ['results_swap.npz', 'content_swap_gt.npz', 'content_swap_test.npz', 'cond_swap_test.npz',
                                    'target_swap_test.npz']}


@pytest.fixture(scope='module')
def inputs():
    base = fixture_dir() + '_evalcli'         # digit-free: the WaveEq split reads the first integer of the path
    shutil.rmtree(base, ignore_errors=True)
    os.makedirs(base)
    try:
        yield {'mnist': I.write_mnist_inputs(os.path.join(base, 'mnist')), 'wave': I.write_wave_inputs(os.path.join(base, 'wave'))}
    finally:
        shutil.rmtree(base, ignore_errors=True)


# ------------------------------------------------------------------------------------------------------------------- the CLIs
@pytest.mark.parametrize('script', ['test', 'test_disentanglement'])
def test_mnist_cli_matches_reference(script, inputs, tmp_path):
    xp = str(tmp_path / 'xp')
    shutil.copytree(os.path.join(GOLDEN_DIR, 'ckpt_dcgan_tiny'), xp)
    shutil.copy(os.path.join(GOLDEN_DIR, 'eval_cli_mnist', 'params.json'), xp)
    out = run_module('test.mnist.%s' % script, ['--xp_dir', xp, '--data_dir', inputs['mnist'], '--nt_pred', str(I.MNIST_RUN['nt_pred']),
                                                  '--batch_size', str(I.MNIST_RUN['batch_size'][script]), '--device', '0'])
    with open(os.path.join(GOLDEN_DIR, 'eval_cli_mnist', 'printed.json')) as f:
        want = json.load(f)[script]
    got = I.parse_results(out)
    assert set(got) == {'mse', 'psnr', 'ssim'} and all(close(got[k], want[k]) for k in want), (got, want)
    for name in OUTPUTS[script]:
        with np.load(os.path.join(xp, name)) as z_got, np.load(os.path.join(GOLDEN_DIR, 'eval_cli_mnist', name)) as z_want:
            assert sorted(z_got.files) == sorted(z_want.files), name
            for key in z_want.files:
                g, w = z_got[key], z_want[key]
                assert g.shape == w.shape and g.dtype == w.dtype, (name, key, g.shape, w.shape, g.dtype, w.dtype)
                if name in DATA_ARRAYS:
                    assert np.array_equal(g, w), (name, key)
                elif name in MODEL_ARRAYS:
                    d = np.abs(g.astype(np.int16) - w.astype(np.int16))
                    assert d.max() <= 1 and np.count_nonzero(d) <= 1e-3 * d.size, (name, key, int(d.max()), np.count_nonzero(d))
                else:
                    assert close(g, w), (name, key, np.abs(g - w).max())


@pytest.mark.parametrize('kind', ['wave', 'wave_partial'])
def test_wave_cli_matches_reference(kind, inputs, tmp_path):
    xp = str(tmp_path / 'xp')
    shutil.copytree(os.path.join(GOLDEN_DIR, 'eval_cli_' + kind), xp)
    out = run_module('test.wave.test', ['--xp_dir', xp, '--data_dir', inputs['wave'], '--batch_size', str(I.WAVE_RUN['batch_size']),
                                       '--device', '0'])
    with open(os.path.join(GOLDEN_DIR, 'eval_cli_' + kind, 'printed.json')) as f:
        want = json.load(f)
    got = I.parse_results(out)
    assert 'mse_t40' in got and close(got['mse_t40'], want['mse_t40'], floor=0), (got, want)


@pytest.mark.parametrize('kind', ['wave', 'wave_partial'])
def test_wave_mse_arrays_match_reference(kind, inputs):
    """Per-window, per-frame MSE ([B, T] / [B, T, 1]) through the CLI's compute_mse, files listed in sorted order as the fixture was."""
    from spatiotemporal_variable_separation_amd.test.wave import test as wave_test
    from spatiotemporal_variable_separation_amd.test.utils import load_model
    from spatiotemporal_variable_separation_amd.utils.helper import load_json
    xp = os.path.join(GOLDEN_DIR, 'eval_cli_' + kind)
    cfg = load_json(os.path.join(xp, 'params.json'))
    cfg.device, cfg.data_dir, cfg.xp_dir, cfg.nt_pred = torch.device('cuda', 0), inputs['wave'], xp, 40
    with sorted_listdir():
        test_set = wave_test.load_dataset(cfg, train=False)
    try:
        mse = np.concatenate(wave_test.compute_mse(cfg, I.WAVE_RUN['batch_size'], test_set, load_model(cfg)), axis=0)
    finally:
        torch.set_grad_enabled(True)
    with np.load(os.path.join(xp, 'mse.npz')) as z:
        want = z['mse']
    assert mse.shape == want.shape == ((len(test_set),) + ((40,) if kind == 'wave' else (40, 1)))
    assert close(mse, want, floor=0), np.abs(mse / want - 1).max()


# ------------------------------------------------------------------------------------------------------------------ the kernels
def _place_case(nd, seed, n_digits=40, T=6, n_seq=7, V=9, F=64):
    rng = np.random.RandomState(seed)
    digits = rng.randint(0, 256, size=(n_digits, 28, 28)).astype(np.uint8)
    pos = rng.randint(0, F - 28 + 1, size=(T, n_seq, nd, 2)).astype(np.int32)
    pos[0, 0, 0] = (F - 28, F - 28)                  # both borders touched exactly
    pos[1, 0, 0] = (0, 0)
    desc = np.concatenate([rng.randint(0, n_seq, size=(V, 1)), rng.randint(0, n_digits, size=(V, nd))], axis=1).astype(np.int32)
    desc[0, 0] = 0
    ref = np.zeros((V, T, 1, F, F), dtype=np.float32)
    for v in range(V):
        for t in range(T):
            for i in range(nd):
                sx, sy = pos[t, desc[v, 0], i]
                ref[v, t, 0, sx:sx + 28, sy:sy + 28] += digits[desc[v, 1 + i]]
    ref[ref > 255] = 255
    return digits, pos, desc, ref / np.float32(255)


@pytest.mark.parametrize('nd', [1, 2, 3])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_moving_mnist_place_bit_exact(nd, dtype):
    from spatiotemporal_variable_separation_amd import ops
    digits, pos, desc, ref = _place_case(nd, 10 + nd)
    T = pos.shape[0]
    out = ops.moving_mnist_place(torch.from_numpy(digits).cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(desc).cuda(), T, 64, dtype)
    assert out.dtype == dtype and tuple(out.shape) == ref.shape
    assert torch.equal(out.cpu(), torch.from_numpy(ref).to(dtype))
    # fewer frames than the table holds
    out = ops.moving_mnist_place(torch.from_numpy(digits).cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(desc).cuda(), T - 2, 64, dtype)
    assert torch.equal(out.cpu(), torch.from_numpy(ref[:, :T - 2]).to(dtype))


def test_swap_dataset_matches_numpy(inputs):
    """SwapDataset.batch against test_disentanglement.py:66-86 restated in NumPy for the same items (n_object = 2)."""
    import itertools
    from spatiotemporal_variable_separation_amd.test.mnist.test_disentanglement import SwapDataset
    data = inputs['mnist']
    np.random.seed(5)
    ds = SwapDataset(data, 7, 3, 2)
    latents = np.load(os.path.join(data, 'mmnist_test_2digits_64.npz'))['latents']
    images = I.read_idx(os.path.join(data, 'MNIST', 'raw', 't10k-images-idx3-ubyte'))
    idx = [0, 1, 4998, 4999]
    cond, target, swap_cond, swap_target = [t.cpu().numpy() for t in ds.batch(idx)]
    for b, index in enumerate(idx):
        rev = np.zeros((7, 1, 64, 64), dtype=np.float32)
        swap = np.zeros((2, 7, 1, 64, 64), dtype=np.float32)
        img = [images[ds.digits_permutation[index + i * 5000]] for i in range(2)]
        for t in range(7):
            for i in range(2):
                sx, sy = latents[t, 5000 - index - 1, i, :2]
                rev[t, 0, sx:sx + 28, sy:sy + 28] += img[i]
            for j, reordering in enumerate(itertools.permutations(range(2))):
                for i in range(2):
                    sx, sy = latents[t, index, i, :2]
                    swap[j, t, 0, sx:sx + 28, sy:sy + 28] += img[reordering[i]]
        rev[rev > 255] = 255
        swap[swap > 255] = 255
        rev, swap = rev / np.float32(255), swap / np.float32(255)
        assert np.array_equal(cond[b], rev[:3]) and np.array_equal(target[b], rev[3:])
        assert np.array_equal(swap_cond[b], swap[:, :3]) and np.array_equal(swap_target[b], swap[:, 3:])


def test_moving_mnist_place_rejects_bad_tables():
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd._lib import VarsepHipError
    digits, pos, desc, _ = _place_case(2, 3)
    d, p, q = torch.from_numpy(digits).cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(desc).cuda()
    for t, s, i, val in ((2, int(desc[0, 0]), 1, (37, 0)), (0, int(desc[0, 0]), 0, (0, -1))):
        bad = p.clone()
        bad[t, s, i] = torch.tensor(val, dtype=torch.int32)
        with pytest.raises(VarsepHipError, match='inside the'):
            ops.moving_mnist_place(d, bad, q, pos.shape[0], 64)
    for col, val in ((0, pos.shape[1]), (1, digits.shape[0]), (2, -1)):
        bad = q.clone()
        bad[1, col] = val
        with pytest.raises(VarsepHipError):
            ops.moving_mnist_place(d, p, bad, pos.shape[0], 64)
    with pytest.raises(VarsepHipError):
        ops.moving_mnist_place(torch.from_numpy(digits), torch.from_numpy(pos), torch.from_numpy(desc), pos.shape[0], 64)
    with pytest.raises(VarsepHipError):                  # more frames than the table holds
        ops.moving_mnist_place(d, p, q, pos.shape[0] + 1, 64)


def _metric_pair(shape, P, seed):
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(shape, generator=g)
    targets = (pred.unsqueeze(1) + 0.3 * torch.randn((shape[0], P) + tuple(shape[1:]), generator=g)).clamp(0, 1)
    return pred, targets


@pytest.mark.parametrize('shape,P', [((3, 5, 1, 64, 64), 2), ((2, 3, 2, 40, 56), 6), ((1, 2, 1, 11, 11), 1)])
def test_frame_metrics_multi_matches_single(shape, P):
    from oracle import ssim_ref
    from spatiotemporal_variable_separation_amd import ops
    pred, targets = _metric_pair(shape, P, 7 + P)
    mse, ssim = ops.frame_metrics_multi(pred.cuda(), targets.cuda())
    assert tuple(mse.shape) == tuple(ssim.shape) == (shape[0], P) + tuple(shape[1:3])
    for p in range(P):
        m1, s1 = ops.frame_metrics(pred.cuda(), targets[:, p].cuda())
        assert torch.allclose(mse[:, p], m1, rtol=2e-5, atol=0)
        assert torch.allclose(ssim[:, p], s1, rtol=2e-5, atol=2e-6)
        ref = ssim_ref.ssim_wrapper(pred, targets[:, p])
        assert torch.allclose(ssim[:, p].cpu(), ref, rtol=2e-5, atol=2e-6)
        ref_mse = (pred - targets[:, p]).pow(2).mean(dim=[3, 4])
        assert torch.allclose(mse[:, p].cpu(), ref_mse, rtol=2e-5)
    m_only, none = ops.frame_metrics_multi(pred.cuda(), targets.cuda(), want_ssim=False)
    assert none is None and torch.equal(m_only, mse)
    none, s_only = ops.frame_metrics_multi(pred.cuda(), targets.cuda(), want_mse=False)
    assert none is None and torch.equal(s_only, ssim)


def test_frame_metrics_multi_limits():
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd._lib import VarsepHipError
    pred, targets = _metric_pair((1, 1, 1, 96, 96), 2, 1)
    with pytest.raises(VarsepHipError, match='LDS'):
        ops.frame_metrics_multi(pred.cuda(), targets.cuda())
    pred, targets = _metric_pair((1, 2, 1, 32, 32), 2, 1)
    with pytest.raises(VarsepHipError):
        ops.frame_metrics_multi(pred, targets)
    with pytest.raises(VarsepHipError):
        ops.frame_metrics_multi(pred.cuda(), targets[:, :, :1].cuda())


def test_frames_to_u8_nhwc_matches_torch_cast():
    from spatiotemporal_variable_separation_amd import ops
    k = torch.arange(256, dtype=torch.float32) / 255                       # exact multiples of 1/255 (the data frames)
    up, down = torch.nextafter(k, torch.full_like(k, 2.)), torch.nextafter(k, torch.full_like(k, -1.))
    vals = torch.cat([k, up[:-1], down[1:], torch.rand(4096, generator=torch.Generator().manual_seed(3)), torch.tensor([0.5, 1.0, 0.0])])
    for C in (1, 3):
        x = vals[:4860].reshape(2, 2, C, 3, -1)
        got = ops.frames_to_u8_nhwc(x.cuda()).cpu()
        assert torch.equal(got, x.mul(255).byte().permute(0, 1, 3, 4, 2))
    x16 = vals[:4860].reshape(1, 1, 1, 12, -1).to(torch.bfloat16)
    assert torch.equal(ops.frames_to_u8_nhwc(x16.cuda()).cpu(), x16.float().mul(255).byte().permute(0, 1, 3, 4, 2))
    odd = torch.rand((1, 3, 1, 5, 7))                                       # a byte count that is not a multiple of 4
    assert torch.equal(ops.frames_to_u8_nhwc(odd.cuda()).cpu(), odd.mul(255).byte().permute(0, 1, 3, 4, 2))


def test_frames_to_u8_nhwc_saturates():
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd._lib import VarsepHipError
    x = torch.tensor([-1.0, -1e-3, -0.0, 1.0 + 1e-6, 1.5, 300.0, float('inf'), float('-inf'), float('nan'), 0.999]).reshape(1, 1, 1, 2, 5)
    got = ops.frames_to_u8_nhwc(x.cuda()).cpu().flatten().tolist()
    assert got == [0, 0, 0, 255, 255, 255, 255, 0, 0, 254]
    with pytest.raises(VarsepHipError):
        ops.frames_to_u8_nhwc(x)

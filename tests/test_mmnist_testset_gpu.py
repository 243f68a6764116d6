"""GPU: vs_moving_mnist_testset (csrc/vs_data.hip) through ops.moving_mnist_testset against the reference's recorded test sets
(tests/golden/mmnist_testset.npz) and the NumPy restatement (tests/mmnist_testset_ref.py); the command line of
preprocessing/mnist/make_test_set.py; `MovingMNIST.generated` and the `generated:` form of the evaluation scripts' --data_dir."""
import os
import shutil

import numpy as np
import pytest
import torch

import eval_cli_inputs as E
import mmnist_testset_inputs as I
import mmnist_testset_ref as R
from cli_util import run_module
from golden_util import GOLDEN_DIR
from guard_util import guarded_ops

pytestmark = pytest.mark.gpu

WHOLE = 512          # from this many videos on, vs_moving_mnist_testset runs one workgroup per video (below: per chunk of frames)


@pytest.fixture(autouse=True)
def forget_generated_sets():
    """`MovingMNIST.generated` keeps its sets for the life of the process: none of a test's may stay in HBM behind it."""
    from spatiotemporal_variable_separation_amd.data import moving_mnist
    yield
    moving_mnist.forget_generated()


@pytest.fixture(scope='module')
def cases():
    """Per case: the stand-in images on the device, the draws of the product's `draw_test_set`, and the reference's arrays (read once)."""
    from spatiotemporal_variable_separation_amd.data.moving_mnist import draw_test_set
    out = {}
    state = np.random.get_state()
    for name, c in I.CASES.items():
        images, labels = I.standins(name)
        _, init = draw_test_set(c['images'], (28, 28), c['frame'], c['speed'], c['digits'], c['seed'])
        want = I.golden(name)
        out[name] = dict(c, images=images, labels=labels, dev=torch.from_numpy(images).cuda(), init=init, want=want,
                         seq=torch.from_numpy(want['sequences']).cuda(), lat=torch.from_numpy(want['latents']).cuda())
    np.random.set_state(state)
    return out


def _mismatches(got, want):
    return int((got != want).sum())


# ------------------------------------------------------------------------------------------------ (a) the reference's bytes
@pytest.mark.parametrize('form', ['chunks', 'whole'])
@pytest.mark.parametrize('name', list(I.CASES))
def test_fixture_parity(name, form, cases):
    """Frames and latents equal the reference's, zero mismatches: uint8 time-major (the file's layout) and fp32 video-major (the layout of
    `MovingMNIST.data`), with several workgroups per video ('chunks': the case's few videos) and with one ('whole': the case's videos
    repeated until there are 512; every repetition must equal the reference)."""
    from spatiotemporal_variable_separation_amd import ops
    c = cases[name]
    n, T, F, nd = c['init'].shape[0], c['seq_len'], c['frame'], c['digits']
    reps = 1 if form == 'chunks' else -(-WHOLE // n)
    assert (n * reps >= WHOLE) == (form == 'whole')
    init = np.tile(c['init'], (reps, 1, 1))
    seq = c['seq'].unsqueeze(1).expand(T, reps, n, 1, F, F)
    lat = c['lat'].unsqueeze(1).expand(T, reps, n, nd, 4)

    frames, latents = ops.moving_mnist_testset(c['dev'], init, T, F)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (T, n * reps, 1, F, F) and frames.is_contiguous()
    assert latents.dtype == torch.int32 and tuple(latents.shape) == (T, n * reps, nd, 4)
    assert _mismatches(frames.view(T, reps, n, 1, F, F), seq) == 0
    assert _mismatches(latents.view(T, reps, n, nd, 4), lat) == 0

    frames32, latents32 = ops.moving_mnist_testset(c['dev'], torch.from_numpy(init).cuda(), T, F, fp32=True, time_major=False)
    assert frames32.dtype == torch.float32 and tuple(frames32.shape) == (n * reps, T, 1, F, F)
    assert _mismatches(frames32.view(reps, n, T, 1, F, F).permute(2, 0, 1, 3, 4, 5), seq.float()) == 0
    assert torch.equal(latents32, latents)

    u8_video_major, _ = ops.moving_mnist_testset(c['dev'], init, T, F, time_major=False)
    assert torch.equal(u8_video_major, frames.transpose(0, 1))
    assert torch.equal(ops.moving_mnist_testset(c['dev'], init, T, F, fp32=True)[0], frames.float())


# ------------------------------------------------------------------------------------------------ (b) frames the vectors do not tile
@pytest.mark.parametrize('F', [30, 29, 28])
def test_odd_frame_sizes_against_the_restatement(F):
    """F = 30: 900 elements, no multiple of 16 (uint8 goes element by element) but of 4 (fp32 vectors cross row ends); F = 29: 841, both
    element by element; F = 28 at zero speed: no room at all (see mmnist_testset_inputs.NO_ROOM), the digits always overlap."""
    from spatiotemporal_variable_separation_amd import ops
    images, _ = I.standins('fast3')
    rng = np.random.RandomState(F)
    n, nd, T, speed = 5, 2, 10, (3 if F > 28 else 0)
    init = np.stack([rng.randint(0, len(images), size=(n, nd)), rng.randint(0, F - 27, size=(n, nd)), rng.randint(0, F - 27, size=(n, nd)),
                     rng.randint(-speed, speed + 1, size=(n, nd)), rng.randint(-speed, speed + 1, size=(n, nd))], axis=2).astype(np.int32)
    seq, lat = R.render(images, init, T, F)
    assert (seq == 255).any()
    dev = torch.from_numpy(images).cuda()
    frames, latents = ops.moving_mnist_testset(dev, init, T, F)
    assert np.array_equal(frames.cpu().numpy(), seq) and np.array_equal(latents.cpu().numpy(), lat)
    frames32, _ = ops.moving_mnist_testset(dev, init, T, F, fp32=True, time_major=False)
    assert np.array_equal(frames32.cpu().numpy(), seq.transpose(1, 0, 2, 3, 4).astype(np.float32))


# ------------------------------------------------------------------------------------------------ (c) nothing outside the outputs
@pytest.mark.parametrize('misalign', [0, 1, 3])
@pytest.mark.parametrize('name,form', [('default', 'chunks'), ('fast3', 'whole'), ('tight', 'chunks')])
def test_outputs_stay_inside_their_windows(name, form, misalign, cases, monkeypatch):
    """`frames` and `latents` between two 4 KiB bands of 0xFF (tests/guard_util.py), aligned and shifted by 1 or 3 elements: the uint8
    frames then start at an odd byte and the fp32 frames 4 or 12 bytes off a 16-byte boundary, which takes the element-wise path."""
    from spatiotemporal_variable_separation_amd import ops
    c = cases[name]
    n, T, F = c['init'].shape[0], c['seq_len'], c['frame']
    reps = 1 if form == 'chunks' else -(-WHOLE // n)
    init = np.tile(c['init'], (reps, 1, 1))
    allocs = guarded_ops(monkeypatch, misalign=misalign)
    frames, latents = ops.moving_mnist_testset(c['dev'], init, T, F)
    frames32, latents32 = ops.moving_mnist_testset(c['dev'], init, T, F, fp32=True, time_major=False)
    assert len(allocs.guards) == 4
    assert frames.data_ptr() % 16 == misalign and frames32.data_ptr() % 16 == 4 * misalign
    allocs.check()
    for g, view in zip(allocs.guards, (frames, latents, frames32, latents32)):
        if view.is_floating_point():         # 0xFF is a value that uint8 frames and int32 speeds can hold
            g.assert_written(view)
    seq = c['seq'].unsqueeze(1).expand(T, reps, n, 1, F, F)
    assert _mismatches(frames.view(T, reps, n, 1, F, F), seq) == 0
    assert _mismatches(frames32.view(reps, n, T, 1, F, F).permute(2, 0, 1, 3, 4, 5), seq.float()) == 0
    assert _mismatches(latents.view(T, reps, n, -1, 4), c['lat'].unsqueeze(1).expand(T, reps, n, c['digits'], 4)) == 0
    assert torch.equal(latents32, latents)


def test_wrapper_refuses_tables_that_leave_the_digits_or_the_frame(cases):
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd._lib import VarsepHipError
    c = cases['default']
    for col, val in ((0, c['images'].shape[0]), (0, -1), (1, 37), (2, -1)):
        bad = c['init'].copy()
        bad[1, 1, col] = val
        with pytest.raises(VarsepHipError, match='init names'):
            ops.moving_mnist_testset(c['dev'], bad, 4, 64)
        with pytest.raises(VarsepHipError, match='init names'):
            ops.moving_mnist_testset(c['dev'], torch.from_numpy(bad).cuda(), 4, 64)
    with pytest.raises(VarsepHipError):
        ops.moving_mnist_testset(c['dev'], c['init'].astype(np.int64), 4, 64)
    with pytest.raises(VarsepHipError, match='LDS'):            # 600 videos: one workgroup each, 8200 frames x 8 B + 784 B > 64 KiB of LDS
        ops.moving_mnist_testset(c['dev'], np.zeros((600, 1, 5), dtype=np.int32), 8200, 28)
    # a digit that fills the frame along an axis and moves along it: the reference never finishes this, the wrapper refuses it
    still = np.zeros((3, 2, 5), dtype=np.int32)
    ops.moving_mnist_testset(c['dev'], still, 4, 28)
    for col in (3, 4):
        moving = still.copy()
        moving[2, 1, col] = -1
        with pytest.raises(VarsepHipError, match='no room'):
            ops.moving_mnist_testset(c['dev'], moving, 4, 28)


def test_a_trajectory_table_near_the_lds_limit(cases):
    """One workgroup per video with 7 000 frames of one digit: 56 000 B of positions + 784 B of digit = 56 784 B of dynamic LDS, between
    the 48 KiB that a static allocation may have and the 64 KiB limit of the entry point.  The 'tight' geometry (a bounce nearly every
    frame), four distinct videos repeated to 512, against the restatement."""
    from spatiotemporal_variable_separation_amd import ops
    c = cases['tight']
    T, F, n, reps = 7000, 32, 4, WHOLE // 4
    seq, lat = R.render(c['images'], c['init'][:n], T, F)
    frames, latents = ops.moving_mnist_testset(c['dev'], np.tile(c['init'][:n], (reps, 1, 1)), T, F)
    assert tuple(frames.shape) == (T, WHOLE, 1, F, F)
    assert _mismatches(frames.view(T, reps, n, 1, F, F), torch.from_numpy(seq).cuda().unsqueeze(1)) == 0
    assert _mismatches(latents.view(T, reps, n, 1, 4), torch.from_numpy(lat).cuda().unsqueeze(1)) == 0
    assert (lat[:, :, 0, :2] != lat[:1, :, 0, :2]).any() and (lat[:, :, 0, 2:] != lat[:1, :, 0, 2:]).any()      # they moved and bounced


# ------------------------------------------------------------------------------------------------ (d) the two generators agree
@pytest.mark.parametrize('name', list(I.CASES))
def test_frames_over_255_equal_the_training_generator(name, cases):
    """The same draws through vs_moving_mnist_batch (fp32, normalised) equal the new raw frames divided by 255 with a device-scalar true
    division, bit for bit."""
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd.data.moving_mnist import MovingMNIST
    c = cases[name]
    T, F = c['seq_len'], c['frame']
    train = MovingMNIST(c['images'], F, 2, T, c['speed'], True, c['digits'], True, device='cuda')
    old = train.render(c['init'])
    new, _ = ops.moving_mnist_testset(c['dev'], c['init'], T, F, fp32=True, time_major=False)
    assert old.shape == new.shape and torch.equal(old, new.div(torch.tensor(255., device='cuda')))


# ------------------------------------------------------------------------------------------------ (e) the command line, end to end
def test_cli_writes_the_reference_file_and_generated_equals_it(tmp_path, cases):
    from spatiotemporal_variable_separation_amd.data.moving_mnist import MovingMNIST
    c = cases['default']
    data = I.write_t10k(str(tmp_path / 'data'), c['images'], c['labels'])
    out = run_module('preprocessing.mnist.make_test_set', ['--data_dir', data, '--seq_len', str(c['seq_len']), '--device', '0'], timeout=120)
    path = os.path.join(data, 'mmnist_test_2digits_64.npz')
    assert out.strip().splitlines()[-1] == 'Saving testset at ' + path
    with np.load(path) as z:
        assert sorted(z.files) == sorted(I.ARRAYS)
        for k in I.ARRAYS:
            assert z[k].dtype == c['want'][k].dtype and z[k].shape == c['want'][k].shape and np.array_equal(z[k], c['want'][k]), k
    np.random.seed(9)
    before = np.random.get_state()[1].copy()
    from_file = MovingMNIST.make_dataset(data, 64, 3, 13, 4, True, 2, False, device='cuda')
    made = MovingMNIST.generated(data, 64, 3, 13, 4, 2, 'cuda', file_seq_len=c['seq_len'])
    assert np.array_equal(np.random.get_state()[1], before)              # the global stream is left as it was found
    assert made.data.dtype == torch.float32 and made.data.shape == from_file.data.shape and torch.equal(made.data, from_file.data)
    assert len(made) == len(from_file) == 12 and not made.train
    assert all(torch.equal(a, b) for a, b in zip(made[5], from_file[5]))
    assert torch.equal(made.latents, c['lat'].int())
    assert np.array_equal(made.test_images.cpu().numpy()[made.digits_idx[:24]].reshape(12, 2, 28, 28), c['want']['digits'])
    again = MovingMNIST.generated(data, 64, 3, 13, 4, 2, 'cuda', file_seq_len=c['seq_len'])
    assert again.data.data_ptr() == made.data.data_ptr()                # generated once per process


# ------------------------------------------------------------------------------------------------ (f) evaluation without the file
def test_eval_cli_on_the_generated_set_equals_the_run_on_the_file(tmp_path):
    """test/mnist/test.py with --data_dir D (after make_test_set.py wrote the file) and with --data_dir generated:D: the same `Results:`
    block and equal output files.  16 stand-in test digits: 8 videos."""
    m = E.MNIST
    rng = np.random.RandomState(77)
    data = str(tmp_path / 'data')
    raw = os.path.join(data, 'MNIST', 'raw')
    I.write_t10k(data, E._digits(16, 28, rng), rng.randint(0, 10, size=16).astype(np.uint8))
    E._write_idx(os.path.join(raw, 'train-images-idx3-ubyte'), E._digits(m['n_train'], 28, rng))
    nt_pred = E.MNIST_RUN['nt_pred']
    run_module('preprocessing.mnist.make_test_set', ['--data_dir', data, '--seq_len', str(3 + nt_pred), '--device', '0'], timeout=120)
    runs = {}
    for tag, data_dir in (('file', data), ('generated', 'generated:' + data)):
        xp = str(tmp_path / ('xp_' + tag))
        shutil.copytree(os.path.join(GOLDEN_DIR, 'ckpt_dcgan_tiny'), xp)
        shutil.copy(os.path.join(GOLDEN_DIR, 'eval_cli_mnist', 'params.json'), xp)
        out = run_module('test.mnist.test', ['--xp_dir', xp, '--data_dir', data_dir, '--nt_pred', str(nt_pred), '--batch_size', '3',
                                             '--device', '0'], timeout=300)
        runs[tag] = (xp, out[out.index('Results:'):])
    assert set(E.parse_results(runs['file'][1])) == {'mse', 'psnr', 'ssim'}
    assert runs['file'][1] == runs['generated'][1]
    for name in ('results.npz', 'predictions.npz', 'gt.npz', 'cond.npz', 'content_swap.npz', 'cond_swap.npz', 'target_swap.npz'):
        with np.load(os.path.join(runs['file'][0], name)) as a, np.load(os.path.join(runs['generated'][0], name)) as b:
            assert sorted(a.files) == sorted(b.files) and all(np.array_equal(a[k], b[k]) for k in a.files), name
    with np.load(os.path.join(runs['file'][0], 'gt.npz')) as a:
        assert a['gt'].shape[0] == 8


def test_disentanglement_cli_on_the_generated_set_equals_the_run_on_the_file(tmp_path):
    """test/mnist/test_disentanglement.py on the file against test/mnist/test_disentanglement_generated.py (the file-free form of that
    script: a module of its own, --data_dir generated:D).  The swap set indexes 10 000 test digits, so the set has 5 000 videos; they are kept
    short (3 + 4 frames) and the batches large (1 000) so that the three child processes stay at a few seconds each (16 s in all on one
    MI355X box; the fixed 10 000 digits of the script set the size)."""
    rng = np.random.RandomState(78)
    data = I.write_t10k(str(tmp_path / 'data'), E._digits(10000, 28, rng), rng.randint(0, 10, size=10000).astype(np.uint8))
    run_module('preprocessing.mnist.make_test_set', ['--data_dir', data, '--seq_len', '7', '--device', '0'], timeout=120)
    runs = {}
    for tag, data_dir in (('file', data), ('generated', 'generated:' + data)):
        xp = str(tmp_path / ('xp_' + tag))
        shutil.copytree(os.path.join(GOLDEN_DIR, 'ckpt_dcgan_tiny'), xp)
        shutil.copy(os.path.join(GOLDEN_DIR, 'eval_cli_mnist', 'params.json'), xp)
        script = 'test.mnist.test_disentanglement' + ('_generated' if tag == 'generated' else '')
        out = run_module(script, ['--xp_dir', xp, '--data_dir', data_dir, '--nt_pred', '4', '--batch_size', '1000', '--device', '0'],
                         timeout=300)
        runs[tag] = (xp, out[out.index('Results:'):])
    assert set(E.parse_results(runs['file'][1])) == {'mse', 'psnr', 'ssim'}
    assert runs['file'][1] == runs['generated'][1]
    for name in ('results_swap.npz', 'content_swap_gt.npz', 'content_swap_test.npz', 'cond_swap_test.npz', 'target_swap_test.npz'):
        with np.load(os.path.join(runs['file'][0], name)) as a, np.load(os.path.join(runs['generated'][0], name)) as b:
            assert sorted(a.files) == sorted(b.files) and all(np.array_equal(a[k], b[k]) for k in a.files), name


def test_swap_set_on_the_generated_set_equals_the_one_on_the_file(tmp_path, monkeypatch):
    """test_disentanglement.py's data, in process, at the 10 000 test digits its swap set indexes: `load_dataset` with --data_dir
    generated:D and `GeneratedSwapDataset` launch the generator ONCE and hold the positions, images and videos that they read from the file under D."""
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd.preprocessing.mnist import make_test_set
    from spatiotemporal_variable_separation_amd.test.mnist.test import load_dataset
    from spatiotemporal_variable_separation_amd.test.mnist.test_disentanglement import SwapDataset
    from spatiotemporal_variable_separation_amd.test.mnist.test_disentanglement_generated import GeneratedSwapDataset
    from spatiotemporal_variable_separation_amd.utils.helper import DotDict
    rng = np.random.RandomState(31)
    data = I.write_t10k(str(tmp_path / 'data'), E._digits(10000, 28, rng), rng.randint(0, 10, size=10000).astype(np.uint8))
    arrays = make_test_set.generate(data, 7, 42, 2, 64, 4, torch.device('cuda', 0))
    np.savez(os.path.join(data, 'mmnist_test_2digits_64.npz'), **arrays)
    launches = []
    real = ops.moving_mnist_testset
    monkeypatch.setattr(ops, 'moving_mnist_testset', lambda *a, **kw: launches.append(1) or real(*a, **kw))
    sets = {}
    for tag, data_dir in (('file', data), ('generated', 'generated:' + data)):
        args = DotDict(data_dir=data_dir, nt_cond=3, nt_pred=4, n_object=2)
        np.random.seed(5)
        test_set = load_dataset(args, train=False, device=torch.device('cuda', 0))
        swap = (GeneratedSwapDataset if tag == 'generated' else SwapDataset)(data_dir, 7, 3, 2, device=torch.device('cuda', 0))
        sets[tag] = (test_set, swap, np.random.randint(1 << 30))
    assert len(launches) == 1
    (f_set, f_swap, f_next), (g_set, g_swap, g_next) = sets['file'], sets['generated']
    assert f_next == g_next and np.array_equal(f_swap.digits_permutation, g_swap.digits_permutation)
    assert tuple(g_set.data.shape) == (5000, 100, 1, 64, 64) and torch.equal(g_set.data[:, :7], f_set.data)
    assert g_swap.positions.dtype == torch.int32 and torch.equal(g_swap.positions, f_swap.positions)
    assert torch.equal(g_swap.images, f_swap.images)
    idx = [0, 1, 2500, 4999]
    assert all(torch.equal(a, b) for a, b in zip(g_swap.batch(idx), f_swap.batch(idx)))

"""GPU: the STOCHASTIC Moving-MNIST test set.  `stochastic_test_set` (data/moving_mnist.py: the permutation on the host, one walk launch from
the stream in HBM, one vs_moving_mnist_testset_place launch) against the reference's recorded sets (tests/golden/smnist_testset.npz) and
the NumPy restatement (tests/smnist_testset_ref.py); vs_moving_mnist_testset_place alone against the deterministic fixture, against
vs_moving_mnist_place, under guard bytes, with bad tables and near the LDS limit; `make_test_set.py --stochastic`, `MovingMNIST.generated(
deterministic=False)`, `test.py --mnist_stochastic` and the content swap's stochastic script."""
import os
import shutil

import numpy as np
import pytest
import torch

import eval_cli_inputs as E
import mmnist_testset_inputs as D
import smnist_testset_inputs as I
import smnist_testset_ref as R
from cli_util import ROOT, run_module
from golden_util import GOLDEN_DIR
from guard_util import guarded_ops
from mmnist_draws_inputs import N, state_words

pytestmark = pytest.mark.gpu

WHOLE = 512          # from this many videos on, the renderer runs one workgroup per video (below: per chunk of frames)


@pytest.fixture(autouse=True)
def forget_generated_sets():
    """`MovingMNIST.generated` keeps its sets for the life of the process: none of a test's may stay in HBM behind it."""
    from spatiotemporal_variable_separation_amd.data import moving_mnist
    yield
    moving_mnist.forget_generated()


@pytest.fixture(scope='module')
def cases():
    """Per case, once: the stand-ins on the device, the reference's arrays, and the product's own generation -- frames (uint8, time-major),
    latents, the permutation and the words of the global stream after it (which is then put back)."""
    from spatiotemporal_variable_separation_amd.data.moving_mnist import stochastic_test_set
    out = {}
    kept = np.random.get_state()
    for name, c in I.CASES.items():
        images, labels = I.standins(name)
        want = I.golden(name)
        dev = torch.from_numpy(images).cuda()
        digits_idx, frames, latents = stochastic_test_set(dev, c['frame'], c['speed'], c['digits'], c['seed'], c['seq_len'])
        words = state_words(np.random)
        n = c['images'] // c['digits']
        out[name] = dict(c, images=images, labels=labels, dev=dev, want=want, n=n, digits_idx=digits_idx, frames=frames, latents=latents, words=words,
                         seq=torch.from_numpy(want['sequences'].copy()).cuda(), lat=torch.from_numpy(want['latents'].copy()).cuda().int(),
                         idx=torch.from_numpy(digits_idx[:n * c['digits']].astype(np.int32)).cuda().view(n, c['digits']))
    np.random.set_state(kept)
    return out


def _mismatches(got, want):
    return int((got != want).sum())


def _compose(images, idx, pos, F):
    """One raw frame: the digits `idx` at the corners `pos`, summed and clipped."""
    x = np.zeros((F, F), dtype=np.int64)
    for i, (r, c) in zip(idx, pos):
        x[r:r + images.shape[1], c:c + images.shape[2]] += images[i]
    return np.minimum(x, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ (a) the reference's bytes
@pytest.mark.parametrize('name', list(I.CASES))
def test_generation_equals_the_fixture(name, cases):
    """One walk launch and one render launch give the reference's file: sequences, latents, labels, digits and the stream's final state."""
    c = cases[name]
    T, F, n, nd = c['seq_len'], c['frame'], c['n'], c['digits']
    assert c['frames'].dtype == torch.uint8 and tuple(c['frames'].shape) == (T, n, 1, F, F) and c['frames'].is_contiguous()
    assert c['latents'].dtype == torch.int32 and tuple(c['latents'].shape) == (T, n, nd, 4)
    assert _mismatches(c['frames'], c['seq']) == 0
    assert _mismatches(c['latents'], c['lat']) == 0
    used = c['digits_idx'][:n * nd]
    assert np.array_equal(c['labels'][used].reshape(n, nd), c['want']['labels'])
    assert np.array_equal(c['images'][used].reshape(n, nd, 28, 28), c['want']['digits'])
    assert int(c['words'][N]) == int(c['want']['final'][N]) and np.array_equal(c['words'][:N], c['want']['final'][:N])


@pytest.mark.parametrize('form', ['chunks', 'whole'])
@pytest.mark.parametrize('name', list(I.CASES))
def test_renderer_equals_the_fixture_in_both_layouts_and_launch_shapes(name, form, cases):
    """The walked positions through ops.moving_mnist_testset_place: uint8 time-major (the file's layout) and fp32 video-major (the layout of
    `MovingMNIST.data`), with several workgroups per video ('chunks': the case's few videos) and with one ('whole': the case's videos
    repeated until there are 512; every repetition must equal the reference)."""
    from spatiotemporal_variable_separation_amd import ops
    c = cases[name]
    T, F, n, nd = c['seq_len'], c['frame'], c['n'], c['digits']
    reps = 1 if form == 'chunks' else -(-WHOLE // n)
    assert (n * reps >= WHOLE) == (form == 'whole')
    positions = c['latents'][..., :2].unsqueeze(1).expand(T, reps, n, nd, 2).reshape(T, reps * n, nd, 2)
    idx = c['idx'].repeat(reps, 1)
    seq = c['seq'].unsqueeze(1).expand(T, reps, n, 1, F, F)

    frames = ops.moving_mnist_testset_place(c['dev'], positions, idx, F)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (T, n * reps, 1, F, F) and frames.is_contiguous()
    assert _mismatches(frames.view(T, reps, n, 1, F, F), seq) == 0
    frames32 = ops.moving_mnist_testset_place(c['dev'], positions, idx, F, fp32=True, time_major=False)
    assert frames32.dtype == torch.float32 and tuple(frames32.shape) == (n * reps, T, 1, F, F)
    assert _mismatches(frames32.view(reps, n, T, 1, F, F).permute(2, 0, 1, 3, 4, 5), seq.float()) == 0
    assert torch.equal(ops.moving_mnist_testset_place(c['dev'], positions, idx, F, time_major=False), frames.transpose(0, 1))
    assert torch.equal(ops.moving_mnist_testset_place(c['dev'], positions, idx, F, fp32=True), frames.float())


# ------------------------------------------------------------------------------------------------ (b) without the walk
@pytest.mark.parametrize('name', list(D.CASES))
def test_positions_of_the_deterministic_fixture_give_its_sequences(name):
    """The renderer alone: the (row, column) of the DETERMINISTIC fixture's latents and its permutation give that fixture's frames."""
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd.data.moving_mnist import draw_test_set
    c = D.CASES[name]
    images, _ = D.standins(name)
    want = D.golden(name)
    kept = np.random.get_state()
    _, init = draw_test_set(c['images'], (28, 28), c['frame'], c['speed'], c['digits'], c['seed'])
    np.random.set_state(kept)
    positions = torch.from_numpy(np.ascontiguousarray(want['latents'][..., :2]).astype(np.int32)).cuda()
    idx = torch.from_numpy(np.ascontiguousarray(init[..., 0])).cuda()
    frames = ops.moving_mnist_testset_place(torch.from_numpy(images).cuda(), positions, idx, c['frame'])
    assert np.array_equal(frames.cpu().numpy(), want['sequences'])


@pytest.mark.parametrize('name', list(I.CASES))
def test_frames_over_255_equal_the_swap_renderer(name, cases):
    """The same tables through vs_moving_mnist_place (fp32, normalised) equal the raw frames divided by 255 with a device-scalar true
    division, bit for bit."""
    from spatiotemporal_variable_separation_amd import ops
    c = cases[name]
    T, F, n, nd = c['seq_len'], c['frame'], c['n'], c['digits']
    positions = c['latents'][..., :2].contiguous()
    desc = torch.cat([torch.arange(n, dtype=torch.int32, device='cuda').view(n, 1), c['idx']], dim=1)
    old = ops.moving_mnist_place(c['dev'], positions, desc, T, F)
    new = ops.moving_mnist_testset_place(c['dev'], positions, c['idx'], F, fp32=True, time_major=False)
    assert old.shape == new.shape and torch.equal(old, new.div(torch.tensor(255., device='cuda')))


# ------------------------------------------------------------------------------------------------ (c) frames the vectors do not tile
@pytest.mark.parametrize('F', [30, 29])
def test_odd_frame_sizes_against_the_restatement(F):
    """F = 30: 900 elements, no multiple of 16 (uint8 goes element by element) but of 4 (fp32 vectors cross row ends: the path whose pixels do
    not share a row); F = 29: 841, both element by element.  Two and one pixels of room: a bounce nearly every frame."""
    from spatiotemporal_variable_separation_amd.data.moving_mnist import stochastic_test_set
    images, labels = I.standins('fast3')
    nd, T, speed, seed = 2, 10, 3, 100 + F
    kept = np.random.get_state()
    try:
        want, words = R.make_test_set(images[:10], labels[:10], seed, T, nd, F, speed)
        dev = torch.from_numpy(images[:10]).cuda()
        _, frames, latents = stochastic_test_set(dev, F, speed, nd, seed, T)
        assert np.array_equal(state_words(np.random), words)
        _, frames32, latents32 = stochastic_test_set(dev, F, speed, nd, seed, T, fp32=True, time_major=False)
    finally:
        np.random.set_state(kept)
    assert (want['sequences'] == 255).any()
    assert np.array_equal(frames.cpu().numpy(), want['sequences']) and np.array_equal(latents.cpu().numpy(), want['latents'])
    assert np.array_equal(frames32.cpu().numpy(), want['sequences'].transpose(1, 0, 2, 3, 4).astype(np.float32))
    assert torch.equal(latents32, latents)


# ------------------------------------------------------------------------------------------------ (d) nothing outside the outputs
@pytest.mark.parametrize('misalign', [0, 1, 3])
@pytest.mark.parametrize('name,form', [('default', 'chunks'), ('fast3', 'whole'), ('tight', 'chunks')])
def test_outputs_stay_inside_their_windows(name, form, misalign, cases, monkeypatch):
    """`frames` between two 4 KiB bands of 0xFF (tests/guard_util.py), aligned and shifted by 1 or 3 elements: the uint8 frames then start
    at an odd byte and the fp32 frames 4 or 12 bytes off a 16-byte boundary, which takes the element-wise path.  The error word is guarded too."""
    from spatiotemporal_variable_separation_amd import ops
    c = cases[name]
    T, F, n, nd = c['seq_len'], c['frame'], c['n'], c['digits']
    reps = 1 if form == 'chunks' else -(-WHOLE // n)
    positions = c['latents'][..., :2].unsqueeze(1).expand(T, reps, n, nd, 2).reshape(T, reps * n, nd, 2)
    idx = c['idx'].repeat(reps, 1)
    allocs = guarded_ops(monkeypatch, misalign=misalign)
    frames = ops.moving_mnist_testset_place(c['dev'], positions, idx, F)
    frames32 = ops.moving_mnist_testset_place(c['dev'], positions, idx, F, fp32=True, time_major=False)
    assert len(allocs.guards) == 4                                           # frames and the error word, twice
    assert frames.data_ptr() % 16 == misalign and frames32.data_ptr() % 16 == 4 * misalign
    allocs.check()
    allocs.guards[2].assert_written(frames32)                                # 0xFF is a value that uint8 frames can hold
    seq = c['seq'].unsqueeze(1).expand(T, reps, n, 1, F, F)
    assert _mismatches(frames.view(T, reps, n, 1, F, F), seq) == 0
    assert _mismatches(frames32.view(reps, n, T, 1, F, F).permute(2, 0, 1, 3, 4, 5), seq.float()) == 0


# ------------------------------------------------------------------------------------------------ (e) tables that name what is not there
@pytest.mark.parametrize('what', ['row_past_the_frame', 'negative_column', 'index_past_the_digits', 'negative_index'])
@pytest.mark.parametrize('fp32', [False, True])
def test_a_bad_entry_sets_the_error_word_and_only_that_digit_is_left_out(what, fp32, cases):
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd._lib import VarsepHipError
    c = cases['default']
    T, F, n = c['seq_len'], c['frame'], c['n']
    positions, idx = c['latents'][..., :2].contiguous().clone(), c['idx'].clone()
    want = c['want']['sequences'].copy()
    t, v, d = 3, 1, 1
    pos, ids = positions.cpu().numpy(), idx.cpu().numpy()
    if what == 'row_past_the_frame':
        positions[t, v, d, 0] = F - 28 + 1                                   # one row too low: the digit would be cut at the border
    elif what == 'negative_column':
        positions[t, v, d, 1] = -1
    else:
        idx[v, d] = c['images'].shape[0] if what == 'index_past_the_digits' else -1
    frames_hit = [t] if what in ('row_past_the_frame', 'negative_column') else range(T)
    for f in frames_hit:                                                      # there the video shows its other digit alone
        want[f, v, 0] = _compose(c['images'], [ids[v, 0]], [pos[f, v, 0]], F)
    assert not np.array_equal(want, c['want']['sequences'])
    with pytest.raises(VarsepHipError, match='does not lie inside|outside'):
        ops.moving_mnist_testset_place(c['dev'], positions, idx, F, fp32=fp32)
    frames = ops.moving_mnist_testset_place(c['dev'], positions, idx, F, fp32=fp32, validate=False)
    assert np.array_equal(frames.cpu().numpy(), want.astype(np.float32) if fp32 else want)
    ops.moving_mnist_testset_place(c['dev'], c['latents'][..., :2].contiguous(), c['idx'], F, fp32=fp32)      # sound tables: the word stays 0


def test_the_entry_point_sets_a_word_of_the_callers_and_leaves_it_alone_on_sound_tables(cases):
    from spatiotemporal_variable_separation_amd import _lib
    c = cases['tight']
    T, F, n, nd = c['seq_len'], c['frame'], c['n'], c['digits']
    positions, idx = c['latents'][..., :2].contiguous(), c['idx'].clone()
    frames = torch.empty((T, n, 1, F, F), dtype=torch.uint8, device='cuda')
    word = torch.full((1,), 7, dtype=torch.int32, device='cuda')
    lib = _lib.load_library()

    def launch():
        _lib.check(lib.vs_moving_mnist_testset_place(c['dev'].data_ptr(), c['dev'].shape[0], 28, 28, positions.data_ptr(), idx.data_ptr(), n, nd, T, F,
                                                     frames.data_ptr(), 0, n * F * F, F * F, word.data_ptr(), _lib.stream_ptr()), 'place')
        return int(word.item())

    assert launch() == 7 and _mismatches(frames, c['seq']) == 0
    idx[n - 1, 0] = 1 << 30
    assert launch() == 1


# ------------------------------------------------------------------------------------------------ (f) the LDS of a workgroup
def test_a_position_table_past_the_lds_limit_is_refused_with_its_sizes(cases):
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd._lib import VarsepHipError
    c = cases['tight']
    # 600 videos: one workgroup each, 8200 frames x 8 B + 784 B of digit > 64 KiB of LDS
    positions = torch.zeros((8200, 600, 1, 2), dtype=torch.int32, device='cuda')
    with pytest.raises(VarsepHipError, match=r'LDS') as e:
        ops.moving_mnist_testset_place(c['dev'], positions, torch.zeros((600, 1), dtype=torch.int32, device='cuda'), 28)
    assert '8200' in str(e.value) and '65600' in str(e.value) and '784' in str(e.value)


def test_a_position_table_near_the_lds_limit(cases):
    """One workgroup per video with 7 000 frames of one digit: 56 000 B of positions + 784 B of digit = 56 784 B of dynamic LDS, between the
    48 KiB that a static allocation may have and the 64 KiB limit of the entry point.  A single digit wholly inside a frame: every frame sums
    to its digit's sum, and sampled frames are compared pixel for pixel."""
    from spatiotemporal_variable_separation_amd import ops
    c = cases['tight']
    T, F, V = 7000, 32, WHOLE
    rng = np.random.RandomState(5)
    pos = rng.randint(0, F - 28 + 1, size=(T, V, 1, 2)).astype(np.int32)
    ids = rng.randint(0, c['images'].shape[0], size=(V, 1)).astype(np.int32)
    frames = ops.moving_mnist_testset_place(c['dev'], torch.from_numpy(pos).cuda(), torch.from_numpy(ids).cuda(), F)
    assert tuple(frames.shape) == (T, V, 1, F, F)
    sums = frames.sum(dim=(2, 3, 4), dtype=torch.int64)
    digit_sums = torch.from_numpy(c['images'].astype(np.int64).sum(axis=(1, 2))).cuda()[torch.from_numpy(ids[:, 0]).long().cuda()]
    assert torch.equal(sums, digit_sums.view(1, V).expand(T, V))
    for t, v in [(0, 0), (T - 1, V - 1), (T - 1, 0), (0, V - 1)] + [(int(rng.randint(T)), int(rng.randint(V))) for _ in range(28)]:
        assert np.array_equal(frames[t, v, 0].cpu().numpy(), _compose(c['images'], ids[v], pos[t, v], F)), (t, v)


# ------------------------------------------------------------------------------------------------ (g) the command line, end to end
def _run_make_test_set(args, compress):
    import subprocess
    import sys
    env = dict(os.environ, VARSEP_NPZ_COMPRESS=compress)
    r = subprocess.run([sys.executable, '-m', 'spatiotemporal_variable_separation_amd.preprocessing.mnist.make_test_set'] + args, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize('compress', ['host', 'device'])
def test_cli_writes_the_s_file_and_generated_equals_it(tmp_path, cases, compress):
    from spatiotemporal_variable_separation_amd.data.moving_mnist import MovingMNIST
    c = cases['default']
    data = I.write_t10k(str(tmp_path / 'data'), c['images'], c['labels'])
    out = _run_make_test_set(['--data_dir', data, '--seq_len', str(c['seq_len']), '--device', '0', '--stochastic'], compress)
    path = os.path.join(data, 'smmnist_test_2digits_64.npz')
    assert out.strip().splitlines()[-1] == 'Saving testset at ' + path
    assert sorted(os.listdir(data)) == ['MNIST', 'smmnist_test_2digits_64.npz']
    with np.load(path) as z:
        assert sorted(z.files) == sorted(I.ARRAYS)
        for k in I.ARRAYS:
            assert z[k].dtype == c['want'][k].dtype and z[k].shape == c['want'][k].shape and np.array_equal(z[k], c['want'][k]), k
    np.random.seed(9)
    before = np.random.get_state()
    from_file = MovingMNIST.make_dataset(data, 64, 3, 13, 4, False, 2, False, device='cuda')
    made = MovingMNIST.generated(data, 64, 3, 13, 4, 2, 'cuda', file_seq_len=c['seq_len'], deterministic=False)
    after = np.random.get_state()
    assert np.array_equal(after[1], before[1]) and after[2] == before[2]    # the global stream is left as it was found
    assert made.data.dtype == torch.float32 and made.data.shape == from_file.data.shape and torch.equal(made.data, from_file.data)
    assert len(made) == len(from_file) == 12 and not made.train and made.deterministic is False
    assert all(torch.equal(a, b) for a, b in zip(made[5], from_file[5]))
    assert torch.equal(made.latents, c['lat'])
    assert np.array_equal(made.test_images.cpu().numpy()[made.digits_idx[:24]].reshape(12, 2, 28, 28), c['want']['digits'])
    again = MovingMNIST.generated(data, 64, 3, 13, 4, 2, 'cuda', file_seq_len=c['seq_len'], deterministic=False)
    assert again.data.data_ptr() == made.data.data_ptr()                    # generated once per process
    other = MovingMNIST.generated(data, 64, 3, 13, 4, 2, 'cuda', file_seq_len=c['seq_len'])
    assert other.deterministic is True and not torch.equal(other.data, made.data)         # the deterministic set is a set of its own


# ------------------------------------------------------------------------------------------------ (h) evaluation
def _xp(tmp_path, tag):
    xp = str(tmp_path / ('xp_' + tag))
    shutil.copytree(os.path.join(GOLDEN_DIR, 'ckpt_dcgan_tiny'), xp)
    shutil.copy(os.path.join(GOLDEN_DIR, 'eval_cli_mnist', 'params.json'), xp)
    return xp


def _same_files(a_dir, b_dir, names):
    for name in names:
        with np.load(os.path.join(a_dir, name)) as a, np.load(os.path.join(b_dir, name)) as b:
            assert sorted(a.files) == sorted(b.files) and all(np.array_equal(a[k], b[k]) for k in a.files), name


def test_eval_cli_with_the_flag_on_the_generated_set_equals_the_run_on_the_s_file(tmp_path):
    """test/mnist/test.py --mnist_stochastic with --data_dir D (after make_test_set.py --stochastic wrote the file) and with --data_dir
    generated:D: the same `Results:` block and equal output files.  16 stand-in test digits: 8 videos, written with the script's default 100
    frames, the length `generated:` builds: a stochastic set of fewer frames is another set, not a prefix (every trajectory starts in the
    stream where the one before it stopped)."""
    m = E.MNIST
    rng = np.random.RandomState(77)
    data = str(tmp_path / 'data')
    raw = os.path.join(data, 'MNIST', 'raw')
    I.write_t10k(data, E._digits(16, 28, rng), rng.randint(0, 10, size=16).astype(np.uint8))
    E._write_idx(os.path.join(raw, 'train-images-idx3-ubyte'), E._digits(m['n_train'], 28, rng))
    nt_pred = E.MNIST_RUN['nt_pred']
    run_module('preprocessing.mnist.make_test_set', ['--data_dir', data, '--device', '0', '--stochastic'], timeout=120)
    assert not os.path.exists(os.path.join(data, 'mmnist_test_2digits_64.npz'))
    runs = {}
    for tag, data_dir in (('file', data), ('generated', 'generated:' + data)):
        xp = _xp(tmp_path, tag)
        out = run_module('test.mnist.test', ['--xp_dir', xp, '--data_dir', data_dir, '--nt_pred', str(nt_pred), '--batch_size', '3',
                                             '--device', '0', '--mnist_stochastic'], timeout=300)
        runs[tag] = (xp, out[out.index('Results:'):])
    assert set(E.parse_results(runs['file'][1])) == {'mse', 'psnr', 'ssim'}
    assert runs['file'][1] == runs['generated'][1]
    _same_files(runs['file'][0], runs['generated'][0],
                ('results.npz', 'predictions.npz', 'gt.npz', 'cond.npz', 'content_swap.npz', 'cond_swap.npz', 'target_swap.npz'))
    with np.load(os.path.join(runs['file'][0], 'gt.npz')) as a:
        assert a['gt'].shape[0] == 8


def test_disentanglement_cli_on_the_generated_stochastic_set_equals_the_run_on_the_s_file(tmp_path):
    """test/mnist/test_disentanglement_stochastic.py (test_disentanglement.py's `main` on the stochastic set; a module of its own) with
    --data_dir D, the `s` file, against --data_dir generated:D.  The swap set indexes 10 000 test digits, so the set has 5 000 videos, and `generated:` builds the 100 frames of the
    script's defaults.  A stochastic set of 7 frames is another set (no prefix of it), and reading 2 GB of file would take the test to a
    minute; so the file holds the default set's arrays cut to the 3 + 4 frames the run reads, written here without compression.  Batches
    of 1 000, as in tests/test_mmnist_testset_gpu.py."""
    from spatiotemporal_variable_separation_amd.preprocessing.mnist import make_test_set
    rng = np.random.RandomState(78)
    data = I.write_t10k(str(tmp_path / 'data'), E._digits(10000, 28, rng), rng.randint(0, 10, size=10000).astype(np.uint8))
    kept = np.random.get_state()
    arrays = make_test_set.generate(data, 100, 42, 2, 64, 4, torch.device('cuda', 0), stochastic=True)
    np.random.set_state(kept)
    np.savez(os.path.join(data, make_test_set.file_name(2, 64, stochastic=True)), sequences=arrays['sequences'][:7], latents=arrays['latents'][:7],
             labels=arrays['labels'], digits=arrays['digits'])
    del arrays
    runs = {}
    for tag, data_dir in (('file', data), ('generated', 'generated:' + data)):
        xp = _xp(tmp_path, tag)
        out = run_module('test.mnist.test_disentanglement_stochastic', ['--xp_dir', xp, '--data_dir', data_dir, '--nt_pred', '4', '--batch_size',
                                                                        '1000', '--device', '0'], timeout=300)
        runs[tag] = (xp, out[out.index('Results:'):])
    assert set(E.parse_results(runs['file'][1])) == {'mse', 'psnr', 'ssim'}
    assert runs['file'][1] == runs['generated'][1]
    _same_files(runs['file'][0], runs['generated'][0],
                ('results_swap.npz', 'content_swap_gt.npz', 'content_swap_test.npz', 'cond_swap_test.npz', 'target_swap_test.npz'))

"""The Moving-MNIST test set without a GPU: the NumPy restatement (tests/mmnist_testset_ref.py) against the reference's recorded outputs
(tests/golden/mmnist_testset.npz, written by tests/make_golden_mmnist_testset.py), `draw_test_set` and `read_mnist_labels` of
data/moving_mnist.py, the command line of preprocessing/mnist/make_test_set.py, the `generated:` form of the evaluation scripts' --data_dir,
and the declaration, binding and argument checks of vs_moving_mnist_testset."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mmnist_testset_inputs as I
import mmnist_testset_ref as R
from spatiotemporal_variable_separation_amd import _lib, ops
from spatiotemporal_variable_separation_amd.data import moving_mnist as M
from spatiotemporal_variable_separation_amd.preprocessing.mnist import make_test_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name', list(I.CASES))
def test_restatement_equals_the_recorded_reference_outputs(name):
    c = I.CASES[name]
    images, labels = I.standins(name)
    want = I.golden(name)
    got = R.make_test_set(images, labels, c['seed'], c['seq_len'], c['digits'], c['frame'], c['speed'])
    n = c['images'] // c['digits']
    assert want['sequences'].shape == (c['seq_len'], n, 1, c['frame'], c['frame']) and want['sequences'].dtype == np.uint8
    assert want['latents'].shape == (c['seq_len'], n, c['digits'], 4) and want['latents'].dtype == np.int64
    assert want['labels'].shape == (n, c['digits']) and want['labels'].dtype == np.uint8
    assert want['digits'].shape == (n, c['digits'], 28, 28) and want['digits'].dtype == np.uint8
    for k in I.ARRAYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, k)
    assert (want['sequences'] == 255).any()
    room = c['frame'] - 28
    assert want['latents'][..., :2].min() >= 0 and want['latents'][..., :2].max() <= room


@pytest.mark.parametrize('name', list(I.CASES))
def test_draw_test_set_reproduces_the_permutation_and_the_first_frame(name):
    c = I.CASES[name]
    images, labels = I.standins(name)
    want = I.golden(name)
    np.random.seed(1)
    digits_idx, init = M.draw_test_set(c['images'], (28, 28), c['frame'], c['speed'], c['digits'], c['seed'])
    n = c['images'] // c['digits']
    assert init.dtype == np.int32 and init.shape == (n, c['digits'], 5) and digits_idx.shape == (c['images'],)
    assert sorted(digits_idx.tolist()) == list(range(c['images']))
    used = digits_idx[:n * c['digits']]
    assert np.array_equal(init[..., 0].reshape(-1), used)
    assert np.array_equal(labels[used].reshape(n, c['digits']), want['labels'])
    assert np.array_equal(images[used].reshape(n, c['digits'], 28, 28), want['digits'])
    assert np.array_equal(init[..., 1:3], want['latents'][0, :, :, :2])       # frame 0: the start position is inside, nothing bounces
    r_idx, r_init = R.draw(c['images'], (28, 28), c['frame'], c['speed'], c['digits'], c['seed'])
    assert np.array_equal(digits_idx, r_idx) and np.array_equal(init, r_init)
    # the global stream, as the reference: the draw reseeds it, so what follows it is the same whatever came before
    after = np.random.randint(1 << 30)
    np.random.seed(2)
    M.draw_test_set(c['images'], (28, 28), c['frame'], c['speed'], c['digits'], c['seed'])
    assert np.random.randint(1 << 30) == after


def test_zero_speed_without_room_is_the_clipped_sum():
    """A 28 x 28 digit in a 28 x 28 frame (mmnist_testset_inputs.NO_ROOM: the reference itself does not finish this geometry when a digit
    moves): at zero speed every frame is the clipped sum of the two digits."""
    images, _ = I.standins(I.NO_ROOM)
    init = np.array([[[0, 0, 0, 0, 0], [1, 0, 0, 0, 0]], [[2, 0, 0, 0, 0], [2, 0, 0, 0, 0]]], dtype=np.int32)
    seq, lat = R.render(images, init, 3, 28)
    want = np.minimum(images[[0, 2]].astype(np.int32) + images[[1, 2]], 255).astype(np.uint8)
    assert np.array_equal(seq, np.broadcast_to(want[None, :, None], (3, 2, 1, 28, 28))) and (seq == 255).any() and not lat.any()


@pytest.mark.parametrize('gz', [False, True])
def test_read_mnist_labels(tmp_path, gz):
    images, labels = I.standins('fast3')
    data = I.write_t10k(str(tmp_path), images, labels, gz=gz)
    got = M.read_mnist_labels(data, train=False)
    assert got.dtype == np.uint8 and np.array_equal(got, labels)
    assert np.array_equal(M.read_mnist_images(data, train=False), images)
    got_images, got_labels = make_test_set.read_test_digits(data)
    assert np.array_equal(got_images, images) and np.array_equal(got_labels, labels)
    with pytest.raises(FileNotFoundError, match='train-labels-idx1-ubyte'):
        M.read_mnist_labels(data, train=True)


def test_read_mnist_labels_refuses_a_bad_magic_and_names_missing_files(tmp_path):
    images, labels = I.standins('tight')
    flat = tmp_path / 'flat'
    flat.mkdir()
    (flat / 't10k-labels-idx1-ubyte').write_bytes(np.array([2051, len(labels)], dtype='>i4').tobytes() + labels.tobytes())
    with pytest.raises(ValueError, match='idx1-ubyte'):
        M.read_mnist_labels(str(flat))
    (flat / 't10k-labels-idx1-ubyte').write_bytes(np.array([2049, len(labels)], dtype='>i4').tobytes() + labels.tobytes())
    assert np.array_equal(M.read_mnist_labels(str(flat)), labels)           # directly under data_dir, as read_mnist_images allows
    with pytest.raises(FileNotFoundError) as e:
        make_test_set.read_test_digits(str(tmp_path / 'empty'))
    assert 't10k-images-idx3-ubyte' in str(e.value) and 't10k-labels-idx1-ubyte' in str(e.value)


def test_parser_carries_the_reference_flags(tmp_path, capsys):
    actions = {a.dest: a for a in make_test_set.build_parser()._actions}
    assert set(actions) - {'help'} == {'data_dir', 'seq_len', 'seed', 'digits', 'frame_size', 'max_speed', 'device'}
    assert actions['data_dir'].required and actions['data_dir'].type is str
    for dest, default in (('seq_len', 100), ('seed', 42), ('digits', 2), ('frame_size', 64), ('max_speed', 4)):
        assert actions[dest].default == default and actions[dest].type is int and not actions[dest].required, dest
    assert actions['device'].default is None and actions['device'].type is int
    args = make_test_set.build_parser().parse_args(['--data_dir', 'x', '--digits', '3', '--device', '1'])
    assert (args.data_dir, args.seq_len, args.seed, args.digits, args.frame_size, args.max_speed, args.device) == ('x', 100, 42, 3, 64, 4, 1)
    with pytest.raises(SystemExit) as e:
        make_test_set.main(['--data_dir', str(tmp_path)])
    assert e.value.code != 0
    err = capsys.readouterr().err
    assert '--device' in err and 'no CPU mode' in err
    assert not os.listdir(str(tmp_path))


def test_generated_prefix_of_the_evaluation_scripts():
    from spatiotemporal_variable_separation_amd.test.mnist import test as cli
    assert cli.split_data_dir('generated:/data/mnist') == ('/data/mnist', True)
    assert cli.split_data_dir('/data/generated:x') == ('/data/generated:x', False)
    assert cli.split_data_dir('data') == ('data', False)
    # the file-free content swap is a script of its own with the flags of test_disentanglement.py
    from spatiotemporal_variable_separation_amd.test.mnist import test_disentanglement as filed, test_disentanglement_generated as made
    flags = lambda p: {a.option_strings[0]: (a.default, a.type, a.required) for a in p._actions if a.option_strings}
    assert flags(made.build_parser()) == flags(filed.build_parser())
    assert issubclass(made.GeneratedSwapDataset, filed.SwapDataset)
    args = made.build_parser().parse_args(['--data_dir', 'generated:d', '--xp_dir', 'x', '--nt_pred', '5'])
    with pytest.raises(RuntimeError, match='no CPU mode'):
        made.main(args)
    assert filed.SwapDataset is not made.GeneratedSwapDataset                # the exchange ends with the run
    args = made.build_parser().parse_args(['--data_dir', 'd', '--xp_dir', 'x', '--nt_pred', '5', '--device', '0'])
    with pytest.raises(ValueError, match='generated:D'):                     # a plain directory means the file, as it does to test.py
        made.main(args)


def test_forget_generated_empties_the_process_cache():
    M._GENERATED['key'] = ('frames', 'latents', 'images', 'idx')
    M.forget_generated()
    assert not M._GENERATED


def test_wrapper_refuses_host_digits():
    digits = torch.zeros((4, 28, 28), dtype=torch.uint8)
    init = np.zeros((2, 2, 5), dtype=np.int32)
    with pytest.raises(_lib.VarsepHipError):
        ops.moving_mnist_testset(digits, init, 4, 64)


def test_entry_point_is_declared_bound_and_checks_its_arguments():
    header = open(os.path.join(ROOT, 'include', 'varsep_hip.h')).read()
    assert re.search(r'\bint vs_moving_mnist_testset\(', header)
    assert 'vs_moving_mnist_testset' in _lib.SIGNATURES
    lib = _lib.load_library()
    assert hasattr(lib, 'vs_moving_mnist_testset')
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(digits=p, n_total=10, dh=28, dw=28, init=p, n_videos=5, nd=2, T=100, F=64, frames=p, fp32=0, st=5 * 4096, sv=4096, latents=None):
        return lib.vs_moving_mnist_testset(digits, n_total, dh, dw, init, n_videos, nd, T, F, frames, fp32, st, sv, latents, None)

    bad = [dict(digits=None), dict(init=None), dict(frames=None),                          # null pointers
           dict(n_total=0), dict(dh=0), dict(n_videos=0), dict(T=0),                       # non-positive sizes
           dict(nd=0), dict(nd=9),                                                         # digits per video outside 1..8
           dict(F=27), dict(dw=65),                                                        # a digit larger than the frame
           dict(st=0), dict(sv=-4096), dict(sv=4095), dict(st=4 * 4096),                   # time-major: frames of a step or steps overlap
           dict(st=4096, sv=99 * 4096), dict(st=4095, sv=100 * 4096)]                      # video-major likewise
    for kwargs in bad:
        assert call(**kwargs) == -1, kwargs
        assert 'vs_moving_mnist_testset' in lib.vs_last_error().decode(), kwargs
    # 1000 videos: one workgroup per video, 8200 frames x 1 digit x 8 B + 784 B of digit > 65536 B of LDS
    assert call(n_videos=1000, nd=1, T=8200, st=1000 * 4096) not in (0, -1)
    message = lib.vs_last_error().decode()
    assert 'vs_moving_mnist_testset' in message and 'LDS' in message and '8200' in message and '65600' in message

"""The STOCHASTIC Moving-MNIST test set without a GPU: the NumPy restatement (tests/smnist_testset_ref.py) against the reference's recorded
outputs (tests/golden/smnist_testset.npz, written by tests/make_golden_smnist_testset.py), the walk's logic (csrc/vs_mmnist_walk_core.h)
compiled for the host and run in its four-draw form from the stream as the permutation leaves it, the declaration, binding and argument
checks of vs_moving_mnist_testset_place, the wrappers' refusals, and the additive flags of the command lines."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import smnist_inputs as SI
import smnist_testset_inputs as I
import smnist_testset_ref as R
from mmnist_draws_inputs import N
from spatiotemporal_variable_separation_amd import _lib, ops
from spatiotemporal_variable_separation_amd.data import moving_mnist as M
from spatiotemporal_variable_separation_amd.preprocessing.mnist import make_test_set
from spatiotemporal_variable_separation_amd.utils.helper import DotDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'vs_moving_mnist_testset_place'
LANES = (3, 64, 256)             # an odd count that divides nothing, one wave, four waves


# ---- the fixture --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(I.CASES))
def test_restatement_equals_the_recorded_reference_outputs_and_final_state(name):
    c = I.CASES[name]
    images, labels = I.standins(name)
    want = I.golden(name)
    watch = SI.Watch(np.random)
    kept = np.random.get_state()
    try:
        got, words = R.make_test_set(images, labels, c['seed'], c['seq_len'], c['digits'], c['frame'], c['speed'], note=watch)
    finally:
        np.random.set_state(kept)
    n = c['images'] // c['digits']
    assert want['sequences'].shape == (c['seq_len'], n, 1, c['frame'], c['frame']) and want['sequences'].dtype == np.uint8
    assert want['latents'].shape == (c['seq_len'], n, c['digits'], 4) and want['latents'].dtype == np.int64
    assert want['labels'].shape == (n, c['digits']) and want['labels'].dtype == np.uint8
    assert want['digits'].shape == (n, c['digits'], 28, 28) and want['digits'].dtype == np.uint8
    for k in I.ARRAYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, k)
    assert want['final'].dtype == np.uint32 and np.array_equal(words, want['final'])
    room = c['frame'] - 28
    assert want['latents'][..., :2].min() >= 0 and want['latents'][..., :2].max() <= room
    assert np.abs(want['latents'][..., 2:]).max() <= c['speed']
    # the case is inside the walk kernel's budgets, and `windows` makes it slide its window more than twice
    assert watch.max_passes <= I.MAX_PASSES and max(watch.outputs) < I.SERIAL_FROM
    if name == 'windows':
        assert sum(watch.outputs) > 2 * I.WINDOW and watch.max_passes >= 9


def test_the_stochastic_set_differs_from_the_deterministic_one_after_the_first_bounce():
    """Same seed, same permutation, same first trajectory start (the first four draws); the speeds part ways at a bounce."""
    import mmnist_testset_inputs as D
    det, sto = D.golden('default'), I.golden('default')
    assert np.array_equal(det['labels'], sto['labels']) and np.array_equal(det['digits'], sto['digits'])
    assert np.array_equal(det['latents'][0, 0, 0], sto['latents'][0, 0, 0])
    assert not np.array_equal(det['latents'], sto['latents'])


# ---- the walk's logic on the host: four prefix draws from the state after the permutation -------------------------------------------------
@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """{lanes: {name: (statuses, calls, state words)}}: 0 is the core's one-lane (serial) form, the others the lanes form."""
    tmp = tmp_path_factory.mktemp('smnist_testset_host')
    cases = [I.walk_case(name) for name in I.CASES]
    plain, _ = SI.compile_host_check(tmp)
    lanes, _ = SI.compile_host_check(tmp, lanes=True)
    out = {0: SI.run_host_check(plain, cases, tmp, lanes=1, tag='serial')}
    for n in LANES:
        out[n] = SI.run_host_check(lanes, cases, tmp, lanes=n)
    return out


@pytest.mark.parametrize('lanes', (0,) + LANES)
@pytest.mark.parametrize('name', list(I.CASES))
def test_core_on_the_host_gives_the_fixture_latents_and_final_state(host, name, lanes):
    c, want = I.CASES[name], I.golden(name)
    statuses, calls, words = host[lanes][name]
    assert statuses == [0]
    n_traj = (c['images'] // c['digits']) * c['digits']
    latents = want['latents'].reshape(c['seq_len'], n_traj, 4)
    assert np.array_equal(calls[0]['latents'], latents)
    assert np.array_equal(calls[0]['positions'], latents[:, :, :2])
    assert np.array_equal(calls[0]['pre'][:, :2], latents[0, :, :2])         # no bounce before the first frame: the start position
    assert int(words[N]) == int(want['final'][N]) and np.array_equal(words[:N], want['final'][:N])


def test_state_after_the_permutation_is_where_the_walk_starts():
    for name, c in I.CASES.items():
        np.random.seed(123)
        before = np.random.get_state()
        digits_idx, words = I.state_after_permutation(name)
        after = np.random.get_state()
        assert np.array_equal(before[1], after[1]) and before[2] == after[2]
        images, labels = I.standins(name)
        used = digits_idx[:(c['images'] // c['digits']) * c['digits']]
        assert np.array_equal(labels[used].reshape(-1, c['digits']), I.golden(name)['labels'])
        assert words.shape == (N + 1,) and I.walk_case(name)['n_pre'] == 4


# ---- the entry point ----------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'varsep_hip.h')).read()
    assert re.search(r'\bint %s\(' % NAME, header)
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 16
    assert hasattr(_lib.load_library(), NAME)
    source = open(os.path.join(ROOT, 'spatiotemporal_variable_separation_amd', 'csrc', 'vs_data.hip')).read()
    assert source.count('mm_compose<OUT, VEC>(') == 2                           # one compositing body for the walking and the placing kernel

def test_entry_point_checks_its_arguments_and_launches_nothing():
    lib = _lib.load_library()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(digits=p, n_total=10, dh=28, dw=28, positions=p, digit_idx=p, n_videos=5, nd=2, T=100, F=64, frames=p, fp32=0, st=5 * 4096, sv=4096,
             bad=None):
        return getattr(lib, NAME)(digits, n_total, dh, dw, positions, digit_idx, n_videos, nd, T, F, frames, fp32, st, sv, bad, None)

    refused = [dict(digits=None), dict(positions=None), dict(digit_idx=None), dict(frames=None),          # null pointers
               dict(n_total=0), dict(dh=0), dict(dw=-1), dict(n_videos=0), dict(T=0),                      # non-positive sizes
               dict(nd=0), dict(nd=9),                                                                     # digits per video outside 1..8
               dict(F=27), dict(dw=65),                                                                    # a digit larger than the frame
               dict(st=0), dict(sv=-4096), dict(sv=4095), dict(st=4 * 4096),                               # time-major: frames overlap
               dict(st=4096, sv=99 * 4096), dict(st=4095, sv=100 * 4096)]                                  # video-major likewise
    for kwargs in refused:
        assert call(**kwargs) == -1, kwargs
        assert NAME in lib.vs_last_error().decode(), kwargs
    assert not any(buf)                                                          # `bad` and every other word: untouched
    # 1000 videos: one workgroup per video, 8200 frames x 1 digit x 8 B + 784 B of digit > 65536 B of LDS
    assert call(n_videos=1000, nd=1, T=8200, st=1000 * 4096) not in (0, -1)
    message = lib.vs_last_error().decode()
    assert NAME in message and 'LDS' in message and '8200' in message and '65600' in message and '784' in message


# ---- the wrappers -------------------------------------------------------------------------------------------------------------------------
def test_wrapper_refuses_cpu_tensors_and_malformed_tables(monkeypatch):
    digits = torch.zeros((4, 28, 28), dtype=torch.uint8)
    positions = torch.zeros((3, 2, 2, 2), dtype=torch.int32)
    idx = torch.zeros((2, 2), dtype=torch.int32)
    with pytest.raises(_lib.VarsepHipError, match='MI355X'):
        ops.moving_mnist_testset_place(digits, positions, idx, 64)
    monkeypatch.setattr(ops, 'require_cuda', lambda *t: None)                    # past the device check, still on the host: nothing is launched
    for d, p, i in ((digits.float(), positions, idx), (digits[0], positions, idx), (digits, positions.long(), idx), (digits, positions[..., :1], idx),
                    (digits, positions[0], idx), (digits, positions[:0], idx), (digits, positions, idx.long()), (digits, positions, idx[:1]),
                    (digits, positions, idx.view(-1)), (digits, positions, torch.zeros((2, 3), dtype=torch.int32))):
        with pytest.raises(_lib.VarsepHipError, match='expected'):
            ops.moving_mnist_testset_place(d, p, i, 64)


def test_generation_refuses_a_digit_that_fills_the_frame_before_it_touches_the_stream():
    np.random.seed(4)
    before = np.random.get_state()
    for shape, frame in (((4, 28, 28), 28), ((4, 28, 20), 28), ((4, 20, 32), 32)):
        with pytest.raises(ValueError, match=r'stochastic Moving MNIST: a \d+ x \d+ digit fills the %d x %d frame along an axis' % (frame, frame)):
            M.stochastic_test_set(torch.zeros(shape, dtype=torch.uint8), frame, 4, 2, 42, 10)
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2] == after[2]


def test_generated_keeps_the_two_variants_apart():
    det = M.MovingMNIST.generated_key('d', 64, 4, 2, 'cuda:0')
    sto = M.MovingMNIST.generated_key('d', 64, 4, 2, 'cuda:0', deterministic=False)
    assert det != sto and det == M.MovingMNIST.generated_key('d', 64, 4, 2, torch.device('cuda', 0), 42, 100, True)
    assert sto != M.MovingMNIST.generated_key('d', 64, 4, 2, 'cuda:0', seed=43, deterministic=False)
    assert det == (os.path.abspath('d'), 64, 4, 2, 42, 100, 'cuda:0')            # the deterministic key is what it was


# ---- the command lines --------------------------------------------------------------------------------------------------------------------
def test_make_test_set_carries_the_flag_and_names_the_file(tmp_path, capsys):
    actions = {a.dest: a for a in make_test_set.build_parser(stochastic=True)._actions}
    assert set(actions) - {'help'} == {'data_dir', 'seq_len', 'seed', 'digits', 'frame_size', 'max_speed', 'device', 'stochastic'}
    assert actions['stochastic'].default is False and actions['stochastic'].nargs == 0 and not actions['stochastic'].required
    args = make_test_set.build_parser(stochastic=True).parse_args(['--data_dir', 'x', '--device', '0'])
    assert args.stochastic is False
    assert make_test_set.build_parser(stochastic=True).parse_args(['--data_dir', 'x', '--stochastic']).stochastic is True
    assert make_test_set.file_name(2, 64) == 'mmnist_test_2digits_64.npz'
    assert make_test_set.file_name(3, 32, stochastic=True) == 'smmnist_test_3digits_32.npz'
    with pytest.raises(SystemExit) as e:                                         # the command line knows the flag, and still needs --device
        make_test_set.main(['--data_dir', str(tmp_path), '--stochastic'])
    assert e.value.code != 0 and 'no CPU mode' in capsys.readouterr().err and not os.listdir(str(tmp_path))


def test_make_dataset_reads_the_s_file(tmp_path, monkeypatch):
    seen = []
    monkeypatch.setattr(np, 'load', lambda path, **kw: seen.append(path) or {'sequences': np.zeros((3, 2, 1, 8, 8), dtype=np.uint8)})
    for deterministic in (True, False):
        M.MovingMNIST.make_dataset(str(tmp_path), 64, 2, 3, 4, deterministic, 2, False, device='cpu')
    assert [os.path.basename(p) for p in seen] == ['mmnist_test_2digits_64.npz', 'smmnist_test_2digits_64.npz']


def test_content_swap_on_the_stochastic_set_is_a_script_of_its_own(monkeypatch):
    """test_disentanglement.py and test_disentanglement_generated.py stay as they are; test_disentanglement_stochastic.py runs the former's
    `main` with the swap set and the test set exchanged, on the `s` file or, with the prefix, on the generated set."""
    from spatiotemporal_variable_separation_amd.test.mnist import test_disentanglement as filed, test_disentanglement_stochastic as sto
    flags = lambda p: {a.option_strings[0]: (a.default, a.type, a.required) for a in p._actions if a.option_strings}
    assert flags(sto.build_parser()) == flags(filed.build_parser())
    assert issubclass(sto.StochasticSwapDataset, filed.SwapDataset)
    args = sto.build_parser().parse_args(['--data_dir', 'generated:d', '--xp_dir', 'x', '--nt_pred', '5'])
    with pytest.raises(RuntimeError, match='no CPU mode'):
        sto.main(args)
    seen = {}

    def fake_main(args):
        filed.load_dataset(DotDict(data_dir='D', nt_cond=3, nt_pred=4, n_object=2, mnist_stochastic=False), train=False, device='cuda')
        seen['swap'] = filed.SwapDataset
        return 'ran'

    monkeypatch.setattr(filed, 'main', fake_main)
    monkeypatch.setattr(M.MovingMNIST, 'make_dataset', classmethod(lambda cls, *a, **k: seen.update(a=a)))
    original = filed.SwapDataset, filed.load_dataset
    assert sto.main(args) == 'ran'
    assert seen['swap'] is sto.StochasticSwapDataset and seen['a'][5] is False           # the `deterministic` of make_dataset
    assert (filed.SwapDataset, filed.load_dataset) == original                           # the exchange ends with the run
    # the swap set reads the `s` file under a plain directory
    loaded = []
    monkeypatch.setattr(np, 'load', lambda path, **kw: loaded.append(path) or {'latents': np.zeros((2, 5000, 2, 4), dtype=np.int64)})
    with pytest.raises(ValueError, match='need >= 7 frames'):
        sto.StochasticSwapDataset('D', 7, 3, 2, device='cpu')
    assert loaded == [os.path.join('D', 'smmnist_test_2digits_64.npz')]


def test_evaluation_script_carries_the_flag_off_by_default():
    import importlib
    mod = importlib.import_module('spatiotemporal_variable_separation_amd.test.mnist.test')
    flags = lambda p: {a.option_strings[0]: a for a in p._actions if a.option_strings}
    plain, full = flags(mod.build_parser()), flags(mod.build_parser(stochastic=True))
    assert set(full) - set(plain) == {'--mnist_stochastic'}
    assert full['--mnist_stochastic'].default is False and full['--mnist_stochastic'].nargs == 0
    base = ['--data_dir', 'd', '--xp_dir', 'x', '--nt_pred', '5']
    assert mod.build_parser(stochastic=True).parse_args(base).mnist_stochastic is False
    assert mod.build_parser(stochastic=True).parse_args(base + ['--mnist_stochastic']).mnist_stochastic is True


def test_only_the_flag_selects_the_stochastic_set_never_the_saved_configuration(monkeypatch):
    from spatiotemporal_variable_separation_amd.test.mnist import test as cli
    seen = []
    monkeypatch.setattr(M.MovingMNIST, 'make_dataset', classmethod(lambda cls, *a, **k: seen.append(('file', a, k))))
    monkeypatch.setattr(M.MovingMNIST, 'generated', classmethod(lambda cls, *a, **k: seen.append(('generated', a, k))))
    saved = DotDict(data_dir='D', nt_cond=3, nt_pred=4, n_object=2, mnist_stochastic=True)        # what `main --mnist_stochastic` saves
    cli.load_dataset(saved, train=False, device='cuda')
    cli.load_dataset(saved, train=False, device='cuda', stochastic=True)
    cli.load_dataset(saved, train=True, device='cuda', stochastic=True)
    saved.data_dir = 'generated:D'
    cli.load_dataset(saved, train=False, device='cuda')
    cli.load_dataset(saved, train=False, device='cuda', stochastic=True)
    cli.load_dataset(saved, train=True, device='cuda', stochastic=True)
    assert [s[0] for s in seen] == ['file', 'file', 'file', 'generated', 'generated', 'file']
    assert [s[1][5] for s in seen if s[0] == 'file'] == [True, False, False, False]              # the `deterministic` of make_dataset
    assert [s[1][7] for s in seen if s[0] == 'file'] == [False, False, True, True]               # its `train`
    assert [s[2]['deterministic'] for s in seen if s[0] == 'generated'] == [True, False]

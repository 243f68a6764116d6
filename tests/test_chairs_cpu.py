"""CPU: the host side of the 3D Chairs data path (data/chairs.py) and of its content-swap CLI (test/chairs/test_disentanglement.py): the
reference's flags (tests/golden/eval_cli_chairs/flags.json, read from the reference's script by tests/make_golden_eval_cli_chairs.py),
no CPU mode, the built-in PNG reader, the item decomposition and the split order."""
import json
import os

import numpy as np
import pytest

import chairs_inputs as I
from golden_util import GOLDEN_DIR

PKG = 'spatiotemporal_variable_separation_amd'


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return I.write_tree(str(tmp_path_factory.mktemp('chairs')))


def _host_only(train, n_objects=None):
    """A Chairs object with the host-side state of a split and no device tensor (the constructor refuses a CPU device)."""
    from spatiotemporal_variable_separation_amd.data.chairs import Chairs
    ds = Chairs.__new__(Chairs)
    ds.train, ds.nt_cond, ds.seq_len, ds.image_size = train, 2, 4, 64
    n = I.N_OBJECTS if n_objects is None else n_objects
    cut = int(n * 0.85)
    ds.start_idx, ds.stop_idx = (0, cut) if train else (cut, n)
    return ds


def test_parser_has_reference_flags():
    from spatiotemporal_variable_separation_amd.test.chairs import test_disentanglement as cli
    with open(os.path.join(GOLDEN_DIR, 'eval_cli_chairs', 'flags.json')) as f:
        flags = json.load(f)
    assert [f[0] for f in flags] == ['--data_dir', '--xp_dir', '--epoch', '--batch_size', '--nt_pred', '--device', '--test_seed']
    actions = {a.option_strings[0]: a for a in cli.build_parser()._actions if a.option_strings}
    for flag, default, typ, required in flags:
        a = actions[flag]
        assert a.default == default, (flag, a.default, default)
        assert a.required == required, flag
        assert (a.type.__name__ if a.type else None) == typ, flag
    extra = set(actions) - {f[0] for f in flags} - {'-h'}
    assert extra == {'--precision'}, extra
    assert actions['--precision'].default == 'fp32' and list(actions['--precision'].choices) == ['fp32', 'bf16']


def test_cli_refuses_cpu_mode(tmp_path):
    from spatiotemporal_variable_separation_amd.test.chairs import test_disentanglement as cli
    args = cli.build_parser().parse_args(['--data_dir', str(tmp_path), '--xp_dir', str(tmp_path), '--nt_pred', '5'])
    assert args.device is None
    with pytest.raises(RuntimeError, match='no CPU mode'):
        cli.main(args)


def test_chairs_refuses_cpu_device(tree):
    from spatiotemporal_variable_separation_amd._lib import VarsepHipError
    from spatiotemporal_variable_separation_amd.data.chairs import Chairs
    from spatiotemporal_variable_separation_amd.test.chairs.test_disentanglement import SwapDataset
    with pytest.raises(VarsepHipError, match='no CPU fallback'):
        Chairs(True, tree, 2, seq_len=4, device='cpu')
    with pytest.raises(ValueError):
        Chairs(True, tree, 2, seq_len=63, device='cpu')
    with pytest.raises(ValueError):
        SwapDataset(False, tree, 2, seq_len=62, device='cpu')


def test_builtin_png_reader_equals_pil(tree):
    Image = pytest.importorskip('PIL.Image')
    from spatiotemporal_variable_separation_amd.data.chairs import read_frame, read_png_rgb8
    for k, name in enumerate(I.object_names()):
        views = I.object_views(k)
        for v in range(I.N_VIEWS):
            path = os.path.join(tree, 'rendered_chairs', name, 'renders', '%d.png' % v)
            with Image.open(path) as im:
                want = np.array(im)
            got = read_png_rgb8(path)
            assert got.dtype == np.uint8 and np.array_equal(got, want), path
            assert np.array_equal(want, views[v]), path
            if v == 0:
                assert np.array_equal(read_frame(path, 64, None), want) and np.array_equal(read_frame(path, 64, Image), want)


def test_builtin_png_reader_all_filter_types(tree, tmp_path):
    """Independent of PIL: the five per-object filter types and the cycling rows decode to the pixels that were written."""
    from spatiotemporal_variable_separation_amd.data.chairs import read_png_rgb8
    for k in range(5):
        path = os.path.join(tree, 'rendered_chairs', I.object_names()[k], 'renders', '7.png')
        assert np.array_equal(read_png_rgb8(path), I.object_views(k)[7])
    rng = np.random.RandomState(3)
    noise = rng.randint(0, 256, size=(64, 64, 3)).astype(np.uint8)          # wrap-around of every filter's arithmetic
    for ftype in (None, 0, 1, 2, 3, 4):
        path = str(tmp_path / ('noise_%s.png' % ftype))
        I.write_png(path, noise, ftype)
        assert np.array_equal(read_png_rgb8(path), noise), ftype


def test_bad_files_raise_value_error_naming_the_file(tmp_path):
    from spatiotemporal_variable_separation_amd.data import chairs
    img = np.zeros((32, 64, 3), dtype=np.uint8)
    small = str(tmp_path / 'small.png')
    I.write_png(small, img)
    garbage = str(tmp_path / 'garbage.png')
    with open(garbage, 'wb') as f:
        f.write(b'not a png at all')
    missing = str(tmp_path / 'missing.png')
    for module in (None, chairs._pil_image()):
        for path in (small, garbage, missing):
            with pytest.raises(ValueError, match=os.path.basename(path)):
                chairs.read_frame(path, 64, module)


def test_descriptors_follow_the_reference_decomposition():
    for train in (True, False):
        ds = _host_only(train)
        n = ds.stop_idx - ds.start_idx
        assert len(ds) == 62 * n and ds.n_objects == n == (5 if train else 2)
        idx = list(range(len(ds)))
        got = ds.descriptors(idx)
        assert got.dtype == np.int32 and got.shape == (len(ds), 2)
        for index in idx:
            q, obj = divmod(index, n)
            q, st = divmod(q, 62)
            assert q == 0 and tuple(got[index]) == (obj, st)
        for bad in (len(ds), len(ds) + 3, -1):
            with pytest.raises(IndexError):
                ds.descriptors([0, bad])
        # per-item overrides, as get_sequence's chosen_idx / chosen_id_st
        over = ds.descriptors([0, n + 1, 61 * n], chosen_idx=[n - 1, 0, 0], chosen_id_st=[5, 61, 0])
        assert over.tolist() == [[n - 1, 5], [0, 61], [0, 0]]
        only_obj = ds.descriptors([0, n + 1, 61 * n], chosen_idx=[n - 1, 0, 0])
        assert only_obj.tolist() == [[n - 1, 0], [0, 1], [0, 61]]
        with pytest.raises(IndexError):
            ds.descriptors([0], chosen_idx=[n])
        with pytest.raises(IndexError):
            ds.descriptors([0], chosen_id_st=[62])


def test_split_and_shuffle_order(tree, monkeypatch):
    """The constructor's listing, shuffle and cut: RandomState(42) on the sorted listing without the .mat entry, 85 % / 15 %."""
    from spatiotemporal_variable_separation_amd.data import chairs
    names = sorted(os.listdir(os.path.join(tree, 'rendered_chairs')))
    assert 'all_chair_names.mat' in names
    names.remove('all_chair_names.mat')
    np.random.RandomState(42).shuffle(names)
    decoded = {}

    class Stop(Exception):
        pass

    def fake_decode(self):                               # the constructor has listed, shuffled and cut; nothing goes to a device
        decoded[self.train] = self.sequences[self.start_idx:self.stop_idx]
        decoded['state'] = (self.sequences, self.start_idx, self.stop_idx)
        raise Stop()

    monkeypatch.setattr(chairs.Chairs, '_decode_split', fake_decode)
    for train in (True, False):
        with pytest.raises(Stop):
            chairs.Chairs(train, tree, 2, seq_len=4, device='cuda')
        sequences, start_idx, stop_idx = decoded['state']
        assert sequences == names
        assert (start_idx, stop_idx) == ((0, 5) if train else (5, 7))
        assert decoded[train] == (names[:5] if train else names[5:])
        assert [n for n, _ in I.split_order(train)] == decoded[train]


def test_decode_uses_a_bounded_pool(tree, monkeypatch):
    from spatiotemporal_variable_separation_amd.data import chairs
    seen = {}
    real = chairs.ThreadPoolExecutor

    def pool(max_workers=None, **kw):
        seen['workers'] = max_workers
        return real(max_workers=max_workers, **kw)

    monkeypatch.setattr(chairs, 'ThreadPoolExecutor', pool)
    monkeypatch.setattr(os, 'cpu_count', lambda: 4096)
    ds = _host_only(False)
    ds.data_root = os.path.join(tree, 'rendered_chairs')
    ds.sequences = [n for n, _ in I.split_order(True)] + [n for n, _ in I.split_order(False)]
    got = ds._decode_split()
    assert 1 <= seen['workers'] <= 16
    assert got.shape == (2, 62, 64, 64, 3) and np.array_equal(got, I.split_frames(False))


def test_header_declares_and_library_exports_the_gather():
    from spatiotemporal_variable_separation_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert 'int vs_chairs_gather(' in open(os.path.join(root, 'include', 'varsep_hip.h')).read()
    _lib.build_library()
    assert hasattr(_lib.load_library(), 'vs_chairs_gather') and 'vs_chairs_gather' in _lib.SIGNATURES

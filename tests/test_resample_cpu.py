"""The 3D Chairs preparation without a GPU: the NumPy restatement of PIL's 8-bit Lanczos resampling (tests/resample_ref.py) against PIL's
recorded outputs (tests/golden/resample) and against live PIL where it imports, `ops.lanczos_coeffs`, the new C entry point's declaration
and argument checks, the gen_chairs command line, the listing rule, `generate` with the launch replaced by the restatement, and the
PNG writer."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import chairs_inputs
import resample_inputs as I
import resample_ref as R
from spatiotemporal_variable_separation_amd import _lib, ops
from spatiotemporal_variable_separation_amd.data import chairs as C
from spatiotemporal_variable_separation_amd.preprocessing.chairs import gen_chairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _extents(name):
    _, (left, upper, right, lower), size = I.CASES[name]
    out_w, out_h = (size, size) if isinstance(size, int) else size
    return (right - left, out_w), (lower - upper, out_h)


@pytest.mark.parametrize('name', list(I.CASES))
def test_restatement_equals_the_recorded_pil_outputs(name):
    shape, box, size = I.CASES[name]
    x = I.case_input(name)
    assert x.shape == shape and x.dtype == np.uint8
    got, want = R.resample(x, box, size), I.golden(name)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), '%d bytes differ' % int((got != want).sum())
    if name == 'a':                                      # the hard-edged image clips at both ends
        assert (want[1] == 0).any() and (want[1] == 255).any()
    if name == 'e':                                      # scale 1: the cropped input
        assert np.array_equal(got, x[:, box[1]:box[3], box[0]:box[2]])


@pytest.mark.parametrize('name', list(I.CASES))
def test_restatement_equals_live_pil(name):
    pytest.importorskip('PIL.Image')
    from make_golden_resample import pil_resample
    _, box, size = I.CASES[name]
    x = I.case_input(name)
    want, _ = pil_resample(x, box, size)
    assert np.array_equal(R.resample(x, box, size), want)


def test_lanczos_coeffs_equal_the_restatement_tables():
    for extent, size in sorted({e for name in I.CASES for e in _extents(name)}):
        k, b = ops.lanczos_coeffs(extent, size)
        rk, rb = R.tables(extent, size)
        assert k.dtype == np.int32 and b.dtype == np.int32 and k.shape == rk.shape and b.shape == (size, 2)
        assert np.array_equal(k, rk) and np.array_equal(b, rb), (extent, size)
        assert np.all(np.abs(k.astype(np.int64).sum(axis=1) - (1 << 22)) <= k.shape[1])
        for xx in range(size):                           # entries beyond a row's taps are 0
            assert not k[xx, b[xx, 1]:].any()
    k, b = ops.lanczos_coeffs(400, 64)
    assert k.shape == (64, 39) and tuple(b[0]) == (0, 22) and tuple(b[-1]) == (378, 22)
    assert k.min() == -105497 and k.max() == 716535
    assert ops.lanczos_coeffs(40, 64)[0].shape[1] == 7
    with pytest.raises(_lib.VarsepHipError):
        ops.lanczos_coeffs(0, 4)


def test_resample_refuses_a_cpu_tensor():
    with pytest.raises(_lib.VarsepHipError):
        ops.resample_lanczos_u8(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), (0, 0, 8, 8), 4)


def test_entry_point_is_declared_bound_and_checks_its_arguments():
    header = open(os.path.join(ROOT, 'include', 'varsep_hip.h')).read()
    assert re.search(r'\bint vs_resample_u8\(', header)
    assert 'vs_resample_u8' in _lib.SIGNATURES and 'vs_resample.hip' in _lib.SOURCES
    lib = _lib.load_library()
    assert hasattr(lib, 'vs_resample_u8')
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(src=p, n=1, H=600, W=600, C=3, box=(100, 100, 400, 400), kx=p, bx=p, ksx=39, ky=p, by=p, ksy=39, out_w=64, out_h=64, out=p):
        return lib.vs_resample_u8(src, n, H, W, C, box[0], box[1], box[2], box[3], kx, bx, ksx, ky, by, ksy, out_w, out_h, out, None)

    bad = [dict(src=None), dict(kx=None), dict(by=None), dict(out=None),                   # null pointers
           dict(n=0), dict(out_w=0), dict(box=(100, 100, 0, 400)),                         # non-positive sizes
           dict(box=(300, 100, 400, 400)), dict(box=(100, 201, 400, 400)), dict(box=(-1, 0, 400, 400)),      # a box outside the image
           dict(C=5), dict(C=0),
           dict(ksx=0), dict(ksy=0),
           dict(n=1 << 31, out_w=64),                                                      # 2^31 images x 4 bands: no grid holds them
           dict(H=4600, box=(100, 100, 400, 4000))]                                        # 4000 rows x 16 columns x 3: over the LDS budget
    for kwargs in bad:
        assert call(**kwargs) == -1, kwargs
        assert 'vs_resample_u8' in lib.vs_last_error().decode(), kwargs
    call(H=4600, box=(100, 100, 400, 4000))
    message = lib.vs_last_error().decode()
    assert 'LDS' in message and '4000' in message and '192000' in message                  # the message names the sizes


def test_gen_chairs_parser_carries_the_reference_flags(tmp_path, capsys):
    actions = {a.dest: a for a in gen_chairs.build_parser()._actions}
    assert actions['data_dir'].required and actions['data_dir'].type is str
    assert actions['image_size'].default == 64 and actions['image_size'].type is int and not actions['image_size'].required
    assert set(actions) - {'help', 'data_dir', 'image_size'} == {'device'}
    args = gen_chairs.build_parser().parse_args(['--data_dir', 'x'])
    assert (args.data_dir, args.image_size, args.device) == ('x', 64, None)
    assert gen_chairs.build_parser().parse_args(['--data_dir', 'x', '--image_size', '32', '--device', '1']).image_size == 32
    with pytest.raises(SystemExit) as e:
        gen_chairs.main(['--data_dir', str(tmp_path)])
    assert e.value.code != 0
    assert '--device' in capsys.readouterr().err


def test_chairs_raw_flag_selects_from_raw(monkeypatch):
    from spatiotemporal_variable_separation_amd import main as M
    from spatiotemporal_variable_separation_amd.options import parser
    from spatiotemporal_variable_separation_amd.test.chairs import test_disentanglement as cli, test_disentanglement_raw as raw_cli
    base = ['--xp_dir', 'x', '--data_dir', 'd', '--data', 'chairs', '--nt_cond', '2', '--nt_pred', '3']
    plain, raw = parser.parse_args(base), parser.parse_args(base + ['--chairs_raw'])
    assert not plain.chairs_raw and raw.chairs_raw and raw.chairs_box == [100, 100, 500, 500]
    assert parser.parse_args(base + ['--chairs_raw', '--chairs_box', '20', '20', '100', '100']).chairs_box == [20, 20, 100, 100]
    calls = []
    monkeypatch.setattr(C.Chairs, '__init__', lambda self, *a, **kw: calls.append((self.raw_box, a, kw)))
    M.load_dataset(plain, torch.device('cuda', 0))
    M.load_dataset(raw, torch.device('cuda', 0))
    assert calls[0] == (None, (True, 'd', 2), dict(seq_len=5, device=torch.device('cuda', 0)))
    assert calls[1] == ((100, 100, 500, 500), (True, 'd', 2), dict(seq_len=5, image_size=64, device=torch.device('cuda', 0)))
    # the evaluation on raw renders is a script of its own: the prepared one's flags plus the box
    flags = lambda p: {a.option_strings[0] for a in p._actions if a.option_strings}
    assert flags(raw_cli.build_parser()) - flags(cli.build_parser()) == {'--chairs_box'}
    args = raw_cli.build_parser().parse_args(['--data_dir', 'd', '--xp_dir', 'x', '--nt_pred', '5'])
    assert args.chairs_box == [100, 100, 500, 500] and args.device is None
    with pytest.raises(RuntimeError, match='no CPU mode'):
        raw_cli.main(args)
    # the content-swap set keeps its own constructor (and its seq_len check) on the raw route
    with pytest.raises(ValueError, match='seq_len < 62'):
        cli.SwapDataset.from_raw(False, 'd', 2, seq_len=62, device='cuda')


def test_listing_skips_the_mat_file_and_prepared_names(tmp_path):
    root = tmp_path / 'rendered_chairs'
    for obj in ('zeta', 'alpha'):
        (root / obj / 'renders').mkdir(parents=True)
    (root / 'all_chair_names.mat').write_bytes(b'x')
    renders = root / 'alpha' / 'renders'
    for f in ('image_010.png', 'image_002.png', '0.png', '17.png', 'b.png', '3.jpg', 'x12.png', '12.png.bak'):
        (renders / f).write_bytes(b'')
    assert C.list_objects(str(tmp_path)) == (str(root), ['alpha', 'zeta'])
    assert C.raw_render_names(str(renders)) == ['12.png.bak', '3.jpg', 'b.png', 'image_002.png', 'image_010.png', 'x12.png']


@pytest.fixture()
def restated(monkeypatch):
    """`ops.resample_lanczos_u8` replaced by the restatement on CPU tensors (the stand-in pattern of tests/ops_standins.py); uploads
    stay on the host and `require_gpu` lets the CPU device through."""
    calls = []

    def stand_in(images_u8, box, size):
        calls.append((tuple(images_u8.shape), tuple(box), size))
        return R.resample_tensor(images_u8, box, size)

    monkeypatch.setattr(ops, 'resample_lanczos_u8', stand_in)
    monkeypatch.setattr(C, 'require_gpu', lambda what, device, hint='': torch.device('cpu'))
    return calls


def _read_all(tree, n_objects, n_views):
    return {(name, i): C.read_png_rgb8(os.path.join(tree, 'rendered_chairs', name, 'renders', '%d.png' % i))
            for name in I.raw_object_names(n_objects) for i in range(n_views)}


def test_generate_writes_the_restated_pixels_and_a_second_run_reproduces_them(tmp_path, restated):
    tree = I.write_raw_tree(tmp_path, 3, 4)
    assert gen_chairs.generate(tree, 64, 'cpu', box=I.RAW_BOX) == 12
    assert restated == [((12, 120, 120, 3), I.RAW_BOX, 64)]           # one launch for the batch of whole objects
    first = _read_all(tree, 3, 4)
    for k, name in enumerate(I.raw_object_names(3)):
        want = R.resample(I.raw_views(k, 4), I.RAW_BOX, 64)
        for i in range(4):
            assert np.array_equal(first[name, i], want[i]), (name, i)
        assert sorted(os.listdir(os.path.join(tree, 'rendered_chairs', name, 'renders'))) == \
            sorted(['%d.png' % i for i in range(4)] + I.raw_file_names(4))
    assert gen_chairs.generate(tree, 64, 'cpu', box=I.RAW_BOX) == 12      # the outputs of the first run are not fed back in
    second = _read_all(tree, 3, 4)
    assert all(np.array_equal(first[key], second[key]) for key in first)
    if C._pil_image() is not None:                                        # PIL wrote them here: the built-in reader agrees with PIL's
        with C._pil_image().open(os.path.join(tree, 'rendered_chairs', I.raw_object_names(3)[0], 'renders', '0.png')) as im:
            assert np.array_equal(np.array(im), first[I.raw_object_names(3)[0], 0])


def test_generate_without_pil_uses_the_built_in_reader_and_writer(tmp_path, restated, monkeypatch):
    monkeypatch.setattr(C, '_pil_image', lambda: None)
    tree = I.write_raw_tree(tmp_path, 2, 3)
    assert gen_chairs.generate(tree, 32, 'cpu', box=I.RAW_BOX) == 6
    got = _read_all(tree, 2, 3)
    for k, name in enumerate(I.raw_object_names(2)):
        want = R.resample(I.raw_views(k, 3), I.RAW_BOX, 32)
        assert all(np.array_equal(got[name, i], want[i]) for i in range(3))


def test_write_png_round_trips(tmp_path):
    rng = np.random.RandomState(5)
    for h, w in ((64, 64), (1, 1), (7, 13)):
        img = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        path = str(tmp_path / ('%dx%d.png' % (h, w)))
        C.write_png_rgb8(path, img)
        assert np.array_equal(C.read_png_rgb8(path), img)
        assert np.array_equal(C.read_frame(path, None), img)
        if C._pil_image() is not None:
            with C._pil_image().open(path) as im:
                assert im.mode == 'RGB' and np.array_equal(np.array(im), img)
    with pytest.raises(ValueError, match='uint8'):
        C.write_png_rgb8(str(tmp_path / 'bad.png'), np.zeros((4, 4), dtype=np.uint8))


def test_read_frame_keeps_its_size_check(tmp_path):
    path = str(tmp_path / 'v.png')
    chairs_inputs.write_png(path, np.zeros((8, 6, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match='64 x 64'):
        C.read_frame(path)
    with pytest.raises(ValueError, match='8 x 8'):
        C.read_frame(path, 8)
    assert C.read_frame(path, None).shape == (8, 6, 3)


@pytest.mark.parametrize('with_pil', [True, False])
def test_bad_sources_raise_naming_the_file(tmp_path, restated, monkeypatch, with_pil):
    if with_pil:
        pytest.importorskip('PIL.Image')
    else:
        monkeypatch.setattr(C, '_pil_image', lambda: None)
    tree = I.write_raw_tree(tmp_path / 'small', 1, 2, size=90)            # 90 x 90: the box (20, 20, 100, 100) is outside
    with pytest.raises(ValueError, match=r'image_00\d\.png.*box'):
        gen_chairs.generate(tree, 64, 'cpu', box=I.RAW_BOX)
    tree = I.write_raw_tree(tmp_path / 'grey', 1, 2)
    grey = os.path.join(tree, 'rendered_chairs', I.raw_object_names(1)[0], 'renders', 'image_001.png')
    raw = open(grey, 'rb').read()
    head = bytearray(raw[:33])
    head[25] = 0                                                          # colour type 0 (greyscale) in IHDR, CRC recomputed
    head[29:33] = (__import__('zlib').crc32(bytes(head[12:29])) & 0xffffffff).to_bytes(4, 'big')
    with open(grey, 'wb') as f:
        f.write(bytes(head) + raw[33:])
    with pytest.raises(ValueError, match='image_001.png'):
        gen_chairs.generate(tree, 64, 'cpu', box=I.RAW_BOX)
    assert not restated                                                   # nothing was launched

"""The 3D Chairs preparation on the device: `ops.resample_lanczos_u8` (vs_resample_u8) byte for byte against the NumPy restatement of PIL's
resampling (tests/resample_ref.py) and against PIL's recorded outputs (tests/golden/resample), `gen_chairs.generate` and its command line,
`Chairs.from_raw` against `Chairs` on a prepared tree, the content-swap evaluation on raw renders, and `main --data chairs --chairs_raw`.  Every
comparison of bytes the resampling decides is exact equality."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import chairs_inputs
import resample_inputs as I
import resample_ref as R
from cli_util import PKG, ROOT, check_training_run, close, run_module

pytestmark = pytest.mark.gpu

N_OBJECTS, N_VIEWS = 7, 62


@pytest.fixture(scope='module')
def expected():
    """name -> the restatement's output of every case, computed once."""
    return {name: R.resample(I.case_input(name), box, size) for name, (_, box, size) in I.CASES.items()}


def _on_device(name):
    from spatiotemporal_variable_separation_amd import ops
    _, box, size = I.CASES[name]
    out = ops.resample_lanczos_u8(torch.from_numpy(I.case_input(name)).cuda(), box, size)
    assert out.dtype == torch.uint8 and out.is_cuda
    return out.cpu().numpy()


@pytest.mark.parametrize('name', list(I.CASES))
def test_kernel_equals_the_restatement_and_the_recorded_pil_outputs(name, expected):
    got = _on_device(name)
    assert got.shape == expected[name].shape
    assert np.array_equal(got, expected[name]), '%d bytes differ from the restatement' % int((got != expected[name]).sum())
    assert np.array_equal(got, I.golden(name)), '%d bytes differ from PIL' % int((got != I.golden(name)).sum())
    if name == 'a':                                      # a second call takes the tables from the cache
        from spatiotemporal_variable_separation_amd import ops
        cached = dict(ops._resample_tables)
        assert np.array_equal(_on_device(name), expected[name])
        assert ops._resample_tables.keys() == cached.keys() and all(ops._resample_tables[k][0] is cached[k][0] for k in cached)


def test_real_shape_in_wide_and_narrow_bands(expected):
    """The launch gives a workgroup 8 output columns when there are few images and 16 otherwise: case (a) has 3 images (narrow bands);
    the same images 22 times over are 66 images x 4 bands = 264 workgroups (wide bands), and every copy must come out the same."""
    from spatiotemporal_variable_separation_amd import ops
    _, box, size = I.CASES['a']
    x = torch.from_numpy(I.case_input('a')).cuda().repeat(22, 1, 1, 1)
    got = ops.resample_lanczos_u8(x, box, size).cpu().numpy()
    assert got.shape == (66, 64, 64, 3)
    assert np.array_equal(got, np.tile(expected['a'], (22, 1, 1, 1)))


def test_kernel_reads_an_unaligned_source(expected):
    """The images start 1 byte into an allocation: the dword loads give way to byte loads, the bytes stay the same."""
    from spatiotemporal_variable_separation_amd import ops
    _, box, size = I.CASES['b']
    x = I.case_input('b')
    flat = torch.empty(x.size + 1, dtype=torch.uint8, device='cuda')
    flat[1:] = torch.from_numpy(x).cuda().reshape(-1)
    view = flat[1:].view(x.shape)
    assert view.data_ptr() % 4 == 1 and view.is_contiguous()
    assert np.array_equal(ops.resample_lanczos_u8(view, box, size).cpu().numpy(), expected['b'])


def test_wild_tables_give_bytes_not_faults():
    """Bounds far outside the box and absurd coefficients: the kernel clamps what it reads, the call returns, the output is defined
    (compared with the same clamping applied on the host)."""
    from spatiotemporal_variable_separation_amd import _lib
    n, H, W, C, ks, ow, oh = 2, 20, 24, 3, 5, 6, 4
    box = (2, 3, 20, 16)                                 # x0, y0, w, h
    rng = np.random.RandomState(11)
    x = rng.randint(0, 256, size=(n, H, W, C)).astype(np.uint8)
    kx = rng.randint(-(1 << 22), 1 << 22, size=(ow, ks)).astype(np.int32)
    ky = rng.randint(-(1 << 22), 1 << 22, size=(oh, ks)).astype(np.int32)
    bx = np.array([[-5, 3], [1000000, 5], [18, 99], [3, -2], [-(1 << 31), (1 << 31) - 1], [19, 1]], dtype=np.int32)
    by = np.array([[15, 7], [-1, 2], [(1 << 31) - 1, (1 << 31) - 1], [0, 5]], dtype=np.int32)

    def clamp(b, extent):
        lo = np.clip(b[:, 0].astype(np.int64), 0, extent)
        return lo, np.clip(b[:, 1].astype(np.int64), 0, np.minimum(ks, extent - lo))

    def one_pass(src, k, lo, cnt):                       # along axis 1, with the kernel's wrapping 32-bit accumulator
        out = np.empty((src.shape[0], k.shape[0]) + src.shape[2:], dtype=np.uint8)
        for i in range(k.shape[0]):
            taps = src[:, lo[i]:lo[i] + cnt[i]].astype(np.int64)
            ss = (1 << 21) + (taps * k[i, :cnt[i]].astype(np.int64).reshape((1, -1) + (1,) * (src.ndim - 2))).sum(axis=1)
            ss = ((ss + (1 << 31)) % (1 << 32)) - (1 << 31)
            out[:, i] = np.clip(ss >> 22, 0, 255)
        return out

    crop = x[:, box[1]:box[1] + box[3], box[0]:box[0] + box[2]]
    tmp = one_pass(crop.transpose(0, 2, 1, 3), kx, *clamp(bx, box[2])).transpose(0, 2, 1, 3)
    want = one_pass(tmp, ky, *clamp(by, box[3]))
    dev = [torch.from_numpy(a).cuda() for a in (x, kx, bx, ky, by)]
    out = torch.full((n, oh, ow, C), 7, dtype=torch.uint8, device='cuda')
    rc = _lib.load_library().vs_resample_u8(dev[0].data_ptr(), n, H, W, C, box[0], box[1], box[2], box[3], dev[1].data_ptr(), dev[2].data_ptr(), ks,
                                            dev[3].data_ptr(), dev[4].data_ptr(), ks, ow, oh, out.data_ptr(), _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------- generate, from_raw, the CLIs
@pytest.fixture(scope='module')
def raw_tree(tmp_path_factory):
    return I.write_raw_tree(tmp_path_factory.mktemp('chairs_raw'), N_OBJECTS, N_VIEWS)


@pytest.fixture(scope='module')
def prepared_tree(tmp_path_factory):
    """A second copy of the raw tree, prepared by `generate` (the raw one stays raw for `from_raw` and `main`)."""
    from spatiotemporal_variable_separation_amd.preprocessing.chairs import gen_chairs
    tree = I.write_raw_tree(tmp_path_factory.mktemp('chairs_prepared'), N_OBJECTS, N_VIEWS)
    assert gen_chairs.generate(tree, 64, torch.device('cuda', 0), box=I.RAW_BOX) == N_OBJECTS * N_VIEWS
    return tree


def test_generate_writes_the_restated_pixels(prepared_tree):
    from spatiotemporal_variable_separation_amd.data.chairs import read_png_rgb8
    for k, name in enumerate(I.raw_object_names(N_OBJECTS)):
        want = R.resample(I.raw_views(k, N_VIEWS), I.RAW_BOX, 64)
        for i in range(N_VIEWS):
            got = read_png_rgb8(os.path.join(prepared_tree, 'rendered_chairs', name, 'renders', '%d.png' % i))
            assert np.array_equal(got, want[i]), (name, i)


@pytest.mark.parametrize('train', [True, False])
def test_from_raw_holds_the_bytes_of_the_prepared_tree(raw_tree, prepared_tree, train):
    from spatiotemporal_variable_separation_amd.data.chairs import Chairs
    files = Chairs(train, prepared_tree, 2, seq_len=5, device='cuda')
    raw = Chairs.from_raw(train, raw_tree, 2, seq_len=5, box=I.RAW_BOX, device='cuda')
    assert raw.sequences == files.sequences and (raw.start_idx, raw.stop_idx) == (files.start_idx, files.stop_idx)
    assert raw.frames.dtype == torch.uint8 and raw.frames.shape == files.frames.shape == (5 if train else 2, 62, 64, 64, 3)
    assert torch.equal(raw.frames, files.frames)
    items = [0, 7, len(files) - 1]
    for a, b in zip(raw.batch(items), files.batch(items)):
        assert torch.equal(a, b)


def test_from_raw_counts_the_renders(raw_tree, tmp_path):
    from spatiotemporal_variable_separation_amd.data.chairs import Chairs
    tree = I.write_raw_tree(tmp_path, N_OBJECTS, 3)
    with pytest.raises(ValueError, match='chair_.*62'):
        Chairs.from_raw(True, tree, 2, seq_len=3, box=I.RAW_BOX, device='cuda')


def test_cli_prepares_full_size_renders(tmp_path):
    """`python -m ...preprocessing.chairs.gen_chairs --data_dir D --device 0` in a fresh process: one object of four 600 x 600 renders
    through the reference's box."""
    from spatiotemporal_variable_separation_amd.data.chairs import read_png_rgb8
    views = I.case_input('a')
    views = np.concatenate([views, views[:1, ::-1]])                      # four renders
    renders = tmp_path / 'rendered_chairs' / 'chair_one' / 'renders'
    renders.mkdir(parents=True)
    (tmp_path / 'rendered_chairs' / 'all_chair_names.mat').write_bytes(b'placeholder')
    for v in range(4):
        chairs_inputs.write_png(str(renders / ('image_%03d.png' % v)), views[v], ftype=v % 3)
    r = subprocess.run(['timeout', '-k', '10', '240', sys.executable, '-m', PKG + '.preprocessing.chairs.gen_chairs', '--data_dir', str(tmp_path),
                        '--device', '0'], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'wrote 4 images of 64 x 64' in r.stdout
    want = R.resample(views, (100, 100, 500, 500), 64)
    for v in range(4):
        assert np.array_equal(read_png_rgb8(str(renders / ('%d.png' % v))), want[v]), v


def test_swap_evaluation_on_raw_renders_equals_the_prepared_one(raw_tree, prepared_tree, tmp_path):
    """`test.chairs.test_disentanglement_raw` on the raw tree and `test.chairs.test_disentanglement` on the prepared one, each in a
    fresh process with the same weights and seed: every output file holds the same bytes."""
    from cli_util import write_xp
    from golden_util import GOLDEN_DIR
    params = os.path.join(GOLDEN_DIR, 'eval_cli_chairs_resnet', 'params.json')
    run = chairs_inputs.RUN
    common = ['--nt_pred', str(run['nt_pred']), '--batch_size', str(run['batch_size']), '--device', '0']
    xp_raw = write_xp('chairs_resnet', str(tmp_path / 'xp_raw'), params)
    xp_files = write_xp('chairs_resnet', str(tmp_path / 'xp_files'), params)
    out_raw = run_module('test.chairs.test_disentanglement_raw', ['--xp_dir', xp_raw, '--data_dir', raw_tree, '--chairs_box'] +
                         [str(v) for v in I.RAW_BOX] + common, timeout=300)
    out_files = run_module('test.chairs.test_disentanglement', ['--xp_dir', xp_files, '--data_dir', prepared_tree] + common, timeout=300)
    assert 'Results:' in out_raw and 'Results:' in out_files
    # the three files of input frames must hold the same bytes: that is what the raw route decides.  The two files computed by the model
    # come from the same inputs and weights in two processes; they are held to the evaluation CLIs' closeness rule (cli_util.close),
    # which allows for a summation order that differs between runs, and are printed when they differ at all
    for name in ('content_swap_gt.npz', 'cond_swap_test.npz', 'target_swap_test.npz', 'results_swap.npz', 'content_swap_test.npz'):
        with np.load(os.path.join(xp_raw, name)) as a, np.load(os.path.join(xp_files, name)) as b:
            assert sorted(a.files) == sorted(b.files) and a.files, name
            for key in a.files:
                if name == 'content_swap_test.npz':        # uint8 frames: the rule of tests/test_chairs_gpu.py
                    d = np.abs(a[key].astype(np.int16) - b[key].astype(np.int16))
                    print(name, key, 'max |diff|', int(d.max()), 'bytes differing', np.count_nonzero(d), 'of', d.size)
                    assert d.max() <= 1 and np.count_nonzero(d) <= 1e-3 * d.size, (name, key)
                elif name == 'results_swap.npz':
                    print(name, key, 'max abs difference', float(np.abs(a[key] - b[key]).max()))
                    assert close(a[key], b[key]), (name, key)
                else:
                    assert np.array_equal(a[key], b[key]), (name, key)


def test_main_trains_on_raw_renders(raw_tree, tmp_path):
    """`main --data chairs --chairs_raw` in a fresh process: 310 train items in two steps (160 and a ragged 150), finite losses, the
    checkpoint files."""
    args = ['--xp_dir', str(tmp_path), '--data_dir', raw_tree, '--chairs_raw', '--chairs_box'] + [str(v) for v in I.RAW_BOX] + \
           ['--device', '0', '--epochs', '1', '--batch_size', '160', '--num_workers', '0', '--seed', '3', '--log_interval', '1', '--chkpt_interval', '1',
            '--data', 'chairs', '--architecture', 'resnet', '--decoder_architecture', 'dcgan', '--nt_cond', '2', '--nt_pred', '2', '--offset', '2',
            '--dec_hidden_size', '8', '--res_hidden_size', '16', '--code_size_s', '12', '--code_size_t', '6', '--lamb_ae', '1', '--lamb_s', '1',
            '--precision', 'bf16']
    check_training_run(run_module('main', args, timeout=900), tmp_path, min_losses=2)

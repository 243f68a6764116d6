"""GPU: the evaluation scripts' result files through the device encoder.  `main` of test/mnist/test.py, test/mnist/test_disentanglement.py
and test/chairs/test_disentanglement.py run twice from the same seed on the stand-ins of tests/eval_cli_inputs.py and tests/chairs_inputs.py,
once per route of VARSEP_NPZ_COMPRESS: the same files, keys, dtypes, shapes and bytes, the same results and the same NumPy stream
afterwards, and on the device route not one call of np.savez_compressed.  The `out=` of ops.frames_to_u8_nhwc, and the writer
(utils/savez.savez_compressed) on a real device tensor that spans slabs."""
import importlib
import os
import shutil
import warnings
import zipfile

import numpy as np
import pytest
import torch

import chairs_inputs as CI
import eval_cli_inputs as I
from golden_util import GOLDEN_DIR

pytestmark = pytest.mark.gpu

FRAME_FILES = {'mnist.test': ['predictions.npz', 'gt.npz', 'cond.npz', 'content_swap.npz', 'cond_swap.npz', 'target_swap.npz'],
               'swap': ['content_swap_gt.npz', 'content_swap_test.npz', 'cond_swap_test.npz', 'target_swap_test.npz']}


@pytest.fixture(scope='module')
def mnist_dir(tmp_path_factory):
    return I.write_mnist_inputs(str(tmp_path_factory.mktemp('evalnpz_mnist')))


@pytest.fixture(scope='module')
def chairs_dir(tmp_path_factory):
    return CI.write_tree(str(tmp_path_factory.mktemp('evalnpz_chairs')))


@pytest.fixture
def restore_process_state():
    """`main` is the body of a command: it switches gradients off for the process."""
    try:
        yield
    finally:
        torch.set_grad_enabled(True)


def _mnist_xp(path):
    shutil.copytree(os.path.join(GOLDEN_DIR, 'ckpt_dcgan_tiny'), path)
    shutil.copy(os.path.join(GOLDEN_DIR, 'eval_cli_mnist', 'params.json'), path)
    return path


def _chairs_xp(path):
    os.makedirs(path)
    for name in ('ov_Es.pt', 'ov_Et.pt', 't_resnet.pt', 'decoder.pt', 'params.json'):
        shutil.copy(os.path.join(GOLDEN_DIR, 'eval_cli_chairs', name), path)
    return path


def _run_both_routes(module, argv, make_xp, tmp_path, monkeypatch):
    """{route: (xp_dir, returned results, NumPy state afterwards, [written files])} of `main` under VARSEP_NPZ_COMPRESS=host and =device;
    on the device route np.savez_compressed raises."""
    mod = importlib.import_module('spatiotemporal_variable_separation_amd.test.' + module)
    from spatiotemporal_variable_separation_amd.utils import savez
    runs = {}
    for route in ('host', 'device'):
        xp = make_xp(str(tmp_path / ('xp_' + route)))
        before = set(os.listdir(xp))
        with monkeypatch.context() as m:
            m.setenv(savez.COMPRESS_ENV, route)
            if route == 'device':
                def refuse(*args, **kwargs):
                    raise AssertionError('np.savez_compressed was called on the device route')
                m.setattr(np, 'savez_compressed', refuse)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')            # (the queue knobs cannot be set once the process has touched the GPU)
                results = mod.main(mod.build_parser().parse_args(['--xp_dir', xp, '--device', '0'] + argv))
        runs[route] = (xp, results, np.random.get_state(), sorted(set(os.listdir(xp)) - before))
    return runs


def _check_equal_runs(runs, frame_files, channels):
    (h_xp, h_res, h_state, h_files), (d_xp, d_res, d_state, d_files) = runs['host'], runs['device']
    assert h_files == d_files and set(frame_files) < set(h_files) and len(h_files) == len(frame_files) + 1
    assert list(h_res) == list(d_res) == ['mse', 'psnr', 'ssim']
    for k in h_res:
        assert h_res[k].dtype == d_res[k].dtype and np.array_equal(h_res[k], d_res[k]), k
    assert h_state[0] == d_state[0] and np.array_equal(h_state[1], d_state[1]) and h_state[2:] == d_state[2:]
    for name in h_files:
        with np.load(os.path.join(h_xp, name), allow_pickle=False) as want, np.load(os.path.join(d_xp, name), allow_pickle=False) as got:
            assert got.files == want.files, name
            for key in want.files:
                g, w = got[key], want[key]
                assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (name, key)
                if name in frame_files:
                    assert g.dtype == np.uint8 and g.ndim == 5 and g.shape[-1] == channels and g.any(), (name, key, g.shape)
        with zipfile.ZipFile(os.path.join(d_xp, name)) as z:
            assert z.testzip() is None, name
            assert all(info.compress_type == zipfile.ZIP_DEFLATED for info in z.infolist()), name


# ------------------------------------------------------------------------------------------------------------------- the scripts
@pytest.mark.parametrize('script', ['test', 'test_disentanglement'])
def test_mnist_scripts_write_the_same_files_on_both_routes(script, mnist_dir, tmp_path, monkeypatch, restore_process_state):
    argv = ['--data_dir', mnist_dir, '--nt_pred', str(I.MNIST_RUN['nt_pred']), '--batch_size', str(I.MNIST_RUN['batch_size'][script])]
    runs = _run_both_routes('mnist.' + script, argv, _mnist_xp, tmp_path, monkeypatch)
    _check_equal_runs(runs, FRAME_FILES['mnist.test' if script == 'test' else 'swap'], channels=1)
    if script == 'test':
        with np.load(os.path.join(runs['device'][0], 'predictions.npz')) as z:
            assert z['predictions'].shape == (I.MNIST['n_videos'], I.MNIST_RUN['nt_pred'], 64, 64, 1)          # 10 chunks of 32 KiB
        with np.load(os.path.join(runs['device'][0], 'cond_swap.npz')) as z:
            assert z.files == ['target_swap']                                # the reference's key for the swap conditioning frames


def test_chairs_script_writes_the_same_files_on_both_routes(chairs_dir, tmp_path, monkeypatch, restore_process_state):
    argv = ['--data_dir', chairs_dir, '--nt_pred', str(CI.RUN['nt_pred']), '--batch_size', str(CI.RUN['batch_size'])]
    runs = _run_both_routes('chairs.test_disentanglement', argv, _chairs_xp, tmp_path, monkeypatch)
    _check_equal_runs(runs, FRAME_FILES['swap'], channels=3)


# ------------------------------------------------------------------------------------------------------------- the converter's out=
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_frames_to_u8_nhwc_writes_into_a_slice_of_a_buffer(dtype):
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd._lib import VarsepHipError
    x = torch.rand((3, 2, 3, 8, 8), generator=torch.Generator().manual_seed(9)).to(dtype).cuda()
    want = ops.frames_to_u8_nhwc(x)
    assert torch.equal(want.cpu(), x.cpu().float().mul(255).byte().permute(0, 1, 3, 4, 2))
    buf = torch.full((7, 2, 8, 8, 3), 0xA5, dtype=torch.uint8, device='cuda')
    got = ops.frames_to_u8_nhwc(x, out=buf[2:5])
    assert got.data_ptr() == buf[2:5].data_ptr() and torch.equal(buf[2:5], want)
    assert bool((buf[:2] == 0xA5).all()) and bool((buf[5:] == 0xA5).all())
    for bad in (buf[2:4], buf[1:5],                                                          # a wrong shape
                torch.empty((3, 2, 8, 8, 3), dtype=torch.int8, device='cuda'),               # a wrong dtype
                torch.empty((3, 2, 8, 8, 3), dtype=torch.uint8),                             # the host
                torch.empty((3, 2, 8, 8, 6), dtype=torch.uint8, device='cuda')[..., ::2],    # not contiguous
                torch.empty((3, 2, 3, 8, 8), dtype=torch.uint8, device='cuda')):             # the input's layout, not NHWC
        with pytest.raises(VarsepHipError):
            ops.frames_to_u8_nhwc(x, out=bad)
    assert torch.equal(buf[2:5], want) and bool((buf[:2] == 0xA5).all()) and bool((buf[5:] == 0xA5).all())


def test_frames_to_u8_nhwc_out_slice_off_a_four_byte_boundary():
    """Frames of 5 x 7 bytes, four at a time: 140 bytes, which the kernel writes as 35 words, into a slice that starts at byte 35."""
    from spatiotemporal_variable_separation_amd import ops
    x = torch.rand((4, 1, 1, 5, 7), generator=torch.Generator().manual_seed(10)).cuda()
    buf = torch.full((6, 1, 5, 7, 1), 0xA5, dtype=torch.uint8, device='cuda')
    assert buf[1:5].data_ptr() % 4 != 0
    ops.frames_to_u8_nhwc(x, out=buf[1:5])
    assert torch.equal(buf[1:5], ops.frames_to_u8_nhwc(x)) and bool((buf[:1] == 0xA5).all()) and bool((buf[5:] == 0xA5).all())


# ---------------------------------------------------------------------------------------------------------------------- the writer
def test_savez_compressed_device_route_on_a_tensor_that_spans_slabs(tmp_path):
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd.utils import savez
    rng = np.random.RandomState(5)
    raw = rng.randint(0, 256, size=3 * ops.DEFLATE_CHUNK + 5).astype(np.uint8)
    floats = rng.standard_normal((4, 3)).astype(np.float32)
    path = str(tmp_path / 'mixed.npz')
    timings = {}
    savez.savez_compressed(path, dict(raw=torch.from_numpy(raw).cuda(), floats=floats, empty=torch.empty((0, 2), dtype=torch.int32, device='cuda')),
                           compress='device', slab_bytes=65536, timings=timings)
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None and z.namelist() == ['raw.npy', 'floats.npy', 'empty.npy']
    with np.load(path, allow_pickle=False) as got:
        assert got.files == ['raw', 'floats', 'empty']
        assert got['raw'].dtype == np.uint8 and np.array_equal(got['raw'], raw)
        assert got['floats'].dtype == np.float32 and np.array_equal(got['floats'], floats)
        assert got['empty'].dtype == np.int32 and got['empty'].shape == (0, 2)
    assert list(timings) == ['write']

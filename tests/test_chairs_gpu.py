"""GPU: the 3D Chairs data path -- vs_chairs_gather (csrc/vs_data.hip), data/chairs.py, `main --data chairs` on a real tree -- and the
content-swap CLI (test/chairs/test_disentanglement.py) against the reference's own outputs on the same inputs
(tests/golden/eval_cli_chairs*, written by tests/make_golden_eval_cli_chairs.py from the tree of tests/chairs_inputs.py)."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import chairs_inputs as I
from cli_util import check_training_run, close, run_module, write_xp
from eval_cli_inputs import parse_results
from golden_util import GOLDEN_DIR

pytestmark = pytest.mark.gpu

DATA_ARRAYS = {'content_swap_gt.npz', 'cond_swap_test.npz', 'target_swap_test.npz'}
MODEL_ARRAYS = {'content_swap_test.npz'}
OUTPUTS = ['results_swap.npz', 'content_swap_gt.npz', 'content_swap_test.npz', 'cond_swap_test.npz', 'target_swap_test.npz']


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return I.write_tree(str(tmp_path_factory.mktemp('chairs')))


# ------------------------------------------------------------------------------------------------------------------ the kernel
def _numpy_gather(frames, desc, seq_len):
    views = frames.shape[1]
    out = np.stack([np.stack([frames[o, (st + t) % views] for t in range(seq_len)]) for o, st in desc])
    return (out / 255).transpose(0, 1, 4, 2, 3).astype(np.float32)          # float64 division, rounded once: the reference's arithmetic


@pytest.mark.parametrize('seq_len', [1, 5, 62])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
def test_chairs_gather_matches_numpy(seq_len, dtype):
    from spatiotemporal_variable_separation_amd import ops
    rng = np.random.RandomState(100 + seq_len)
    frames = rng.randint(0, 256, size=(3, 62, 64, 64, 3)).astype(np.uint8)
    desc = np.array([[0, 0], [2, 61], [1, 60], [2, 30], [0, 58], [1, 1], [2, 0]], dtype=np.int32)          # rows that wrap around and not
    ref = torch.from_numpy(_numpy_gather(frames, desc, seq_len))
    out = ops.chairs_gather(torch.from_numpy(frames).cuda(), torch.from_numpy(desc).cuda(), seq_len, dtype)
    assert out.dtype == dtype and tuple(out.shape) == (len(desc), seq_len, 3, 64, 64)
    assert torch.equal(out.cpu(), ref.to(dtype))          # fp32: bit-identical; 16-bit: torch's cast of the fp32 result


@pytest.mark.parametrize('shape', [(5, 7, 3), (6, 6, 1), (4, 4, 4), (8, 8, 3), (3, 4, 3)])
def test_chairs_gather_other_frame_shapes(shape):
    """Frames that do not take the 3-channel vector form (other channel counts, pixel counts not a multiple of 4 / 8)."""
    from spatiotemporal_variable_separation_amd import ops
    H, W, C = shape
    rng = np.random.RandomState(H * 100 + W * 10 + C)
    frames = rng.randint(0, 256, size=(4, 9, H, W, C)).astype(np.uint8)
    desc = np.array([[3, 8], [0, 0], [1, 4]], dtype=np.int32)
    ref = torch.from_numpy(_numpy_gather(frames, desc, 11))               # seq_len above the view count: wraps more than once
    for dtype in (torch.float32, torch.bfloat16):
        out = ops.chairs_gather(torch.from_numpy(frames).cuda(), torch.from_numpy(desc).cuda(), 11, dtype)
        assert torch.equal(out.cpu(), ref.to(dtype)), (shape, dtype)


def test_chairs_gather_all_byte_values():
    from spatiotemporal_variable_separation_amd import ops
    u8 = np.arange(256, dtype=np.uint8)
    frames = np.zeros((1, 2, 64, 64, 3), dtype=np.uint8)
    frames[0, 0].reshape(-1)[:] = np.resize(u8, 64 * 64 * 3)
    frames[0, 1].reshape(-1)[:] = np.resize(u8[::-1], 64 * 64 * 3)
    out = ops.chairs_gather(torch.from_numpy(frames).cuda(), torch.tensor([[0, 0]], dtype=torch.int32).cuda(), 2).cpu()
    want = torch.tensor(frames[0] / 255).permute(0, 3, 1, 2).float()          # chairs.py:63
    assert set(np.unique(frames)) == set(range(256))
    assert torch.equal(out[0], want)
    assert np.array_equal(out[0].numpy().view(np.uint32), want.numpy().view(np.uint32))


def test_chairs_gather_flags_bad_descriptors():
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd._lib import VarsepHipError
    rng = np.random.RandomState(9)
    frames = rng.randint(1, 256, size=(3, 62, 64, 64, 3)).astype(np.uint8)          # no zero byte: a zeroed row is recognisable
    f = torch.from_numpy(frames).cuda()
    good = np.array([[0, 3], [2, 61], [1, 0]], dtype=np.int32)
    for row, col, val in ((1, 0, 3), (1, 0, -1), (0, 1, 62), (2, 1, -1), (1, 0, 2 ** 31 - 1)):
        desc = good.copy()
        desc[row, col] = val
        d = torch.from_numpy(desc).cuda()
        with pytest.raises(VarsepHipError, match='descriptor'):
            ops.chairs_gather(f, d, 4)
        for dtype in (torch.float32, torch.bfloat16):
            out = ops.chairs_gather(f, d, 4, dtype, validate=False).cpu()
            ref = torch.from_numpy(_numpy_gather(frames, good, 4)).to(dtype)
            assert torch.count_nonzero(out[row]) == 0
            keep = [r for r in range(3) if r != row]
            assert torch.equal(out[keep], ref[keep])
    with pytest.raises(VarsepHipError):
        ops.chairs_gather(torch.from_numpy(frames), torch.from_numpy(good), 4)
    with pytest.raises(VarsepHipError):
        ops.chairs_gather(f, torch.from_numpy(good).cuda().long(), 4)


def test_chairs_gather_argument_checks():
    """Every argument-check path of the C entry point returns VS_ERR_ARG with a message and launches nothing."""
    from spatiotemporal_variable_separation_amd import _lib, ops
    lib = _lib.load_library()
    f = torch.zeros((2, 3, 4, 4, 3), dtype=torch.uint8).cuda()
    d = torch.zeros((2, 2), dtype=torch.int32).cuda()
    out = torch.full((2, 2, 3, 4, 4), 7.0).cuda()
    good = dict(frames=f.data_ptr(), n=2, views=3, H=4, W=4, C=3, desc=d.data_ptr(), rows=2, seq_len=2, out=out.data_ptr(), dtype=_lib.F32)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vs_chairs_gather(a['frames'], a['n'], a['views'], a['H'], a['W'], a['C'], a['desc'], a['rows'], a['seq_len'], a['out'],
                                    a['dtype'], None, _lib.stream_ptr())

    cases = [dict(frames=None), dict(desc=None), dict(out=None), dict(n=0), dict(n=-1), dict(views=0), dict(H=0), dict(W=-2), dict(C=0),
             dict(rows=0), dict(rows=65536), dict(seq_len=0), dict(seq_len=-3), dict(dtype=3), dict(dtype=-1), dict(H=1 << 15, W=1 << 15, C=3)]
    for kw in cases:
        assert call(**kw) != 0, kw
        assert b'vs_chairs_gather' in lib.vs_last_error(), kw
    torch.cuda.synchronize()
    assert torch.all(out == 7.0)                         # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.count_nonzero(out) == 0
    with pytest.raises(_lib.VarsepHipError):
        ops.chairs_gather(f, d, 0)
    with pytest.raises(_lib.VarsepHipError):
        ops.chairs_gather(f, d, 2, torch.float64)


# ----------------------------------------------------------------------------------------------------------------- the dataset
@pytest.mark.parametrize('train', [True, False])
def test_chairs_items_match_numpy(tree, train):
    from spatiotemporal_variable_separation_amd.data.chairs import Chairs
    frames = I.split_frames(train)
    ds = Chairs(train, tree, 2, seq_len=6, device='cuda')
    assert ds.device_resident and ds.max_length == 62 and len(ds) == 62 * frames.shape[0]
    assert ds.frames.dtype == torch.uint8 and np.array_equal(ds.frames.cpu().numpy(), frames)
    idx = [0, 1, frames.shape[0], len(ds) - 1, len(ds) // 2, 57 * frames.shape[0] + 1]           # the last ones wrap past view 61
    cond, target = ds.batch(idx)
    assert tuple(cond.shape) == (len(idx), 2, 3, 64, 64) and tuple(target.shape) == (len(idx), 4, 3, 64, 64)
    for b, index in enumerate(idx):
        want = I.expected_item(frames, index, 6)
        assert np.array_equal(cond[b].cpu().numpy(), want[:2]) and np.array_equal(target[b].cpu().numpy(), want[2:])
        c1, t1 = ds[index]
        assert torch.equal(c1, cond[b]) and torch.equal(t1, target[b])
    c16, t16 = ds.batch(idx, torch.bfloat16)
    assert torch.equal(c16, cond.to(torch.bfloat16)) and torch.equal(t16, target.to(torch.bfloat16))
    with pytest.raises(IndexError):
        ds.batch([len(ds)])


def test_swap_dataset_matches_numpy(tree):
    """SwapDataset.batch against the reference's `__getitem__` restated in NumPy, with the same draws from the global stream."""
    from spatiotemporal_variable_separation_amd.test.chairs.test_disentanglement import SwapDataset
    frames = I.split_frames(False)
    ds = SwapDataset(False, tree, 2, seq_len=5, device='cuda')
    idx = [0, 1, 2, 77, 123]
    np.random.seed(11)
    cond, target, gt_cond, gt_target = [t.cpu().numpy() for t in ds.batch(idx)]
    assert gt_cond.shape == (5, 1, 2, 3, 64, 64) and gt_target.shape == (5, 1, 3, 3, 64, 64)
    np.random.seed(11)
    for b, index in enumerate(idx):
        idx_content = np.random.randint(2)
        id_st_content = np.random.randint(62 - 5)
        seq = I.expected_item(frames, index, 5, chosen_idx=idx_content, chosen_id_st=id_st_content)
        swap = I.expected_item(frames, index, 5, chosen_idx=idx_content)
        assert np.array_equal(cond[b], seq[:2]) and np.array_equal(target[b], seq[2:])
        assert np.array_equal(gt_cond[b, 0], swap[:2]) and np.array_equal(gt_target[b, 0], swap[2:])


def test_device_loader_visits_the_dataloader_items(tree):
    """DeviceBatchLoader(Chairs) under a fixed torch.manual_seed yields the items `DataLoader(shuffle=True)` would: a DataLoader iterator
    draws its base seed, then its RandomSampler draws the permutation."""
    from torch.utils.data import BatchSampler, RandomSampler
    from spatiotemporal_variable_separation_amd.data.chairs import Chairs
    from spatiotemporal_variable_separation_amd.data.device import DeviceBatchLoader
    frames = I.split_frames(True)
    ds = Chairs(True, tree, 2, seq_len=4, device='cuda')
    torch.manual_seed(17)
    torch.empty((), dtype=torch.int64).random_()          # _BaseDataLoaderIter.__init__: the base seed
    want = list(BatchSampler(RandomSampler(ds), 64, False))
    assert sorted(i for b in want for i in b) == list(range(310)) and len(want[-1]) == 310 % 64
    torch.manual_seed(17)
    got = list(DeviceBatchLoader(ds, 64, shuffle=True))
    assert len(got) == len(want)
    for (cond, target), items in zip(got, want):
        assert cond.shape[0] == len(items)
        for b in (0, len(items) - 1):
            ref = I.expected_item(frames, items[b], 4)
            assert np.array_equal(cond[b].cpu().numpy(), ref[:2]) and np.array_equal(target[b].cpu().numpy(), ref[2:])


# --------------------------------------------------------------------------------------------------------------------- the CLI
def _check_cli(case, xp, tree):
    golden = os.path.join(GOLDEN_DIR, case)
    out = run_module('test.chairs.test_disentanglement', ['--xp_dir', xp, '--data_dir', tree, '--nt_pred', str(I.RUN['nt_pred']),
                                                          '--batch_size', str(I.RUN['batch_size']), '--device', '0'], timeout=900)
    with open(os.path.join(golden, 'printed.json')) as f:
        want = json.load(f)
    got = parse_results(out)
    print(case, 'printed', got, 'reference', want)
    for name in OUTPUTS:
        z_got, z_want = I.load_output(xp, name), I.load_output(golden, name)
        assert sorted(z_got) == sorted(z_want), name
        for key in z_want:
            g, w = z_got[key], z_want[key]
            assert g.shape == w.shape and g.dtype == w.dtype, (name, key, g.shape, w.shape, g.dtype, w.dtype)
            if name in DATA_ARRAYS:
                assert np.array_equal(g, w), (name, key)
            elif name in MODEL_ARRAYS:
                d = np.abs(g.astype(np.int16) - w.astype(np.int16))
                print(case, name, 'max |diff|', int(d.max()), 'bytes differing', np.count_nonzero(d), 'of', d.size)
                assert d.max() <= 1 and np.count_nonzero(d) <= 1e-3 * d.size, (name, key, int(d.max()), np.count_nonzero(d))
            else:
                print(case, name, key, 'max rel', float(np.max(np.abs(g - w) / np.abs(w))))
                assert close(g, w), (name, key, np.abs(g - w).max())
    assert set(got) == {'mse', 'psnr', 'ssim'} and all(close(got[k], want[k]) for k in want), (got, want)


def test_chairs_cli_matches_reference(tree, tmp_path):
    """The reference-written checkpoint of a small 3-channel DCGAN network."""
    xp = str(tmp_path / 'xp')
    os.makedirs(xp)
    for name in ('ov_Es.pt', 'ov_Et.pt', 't_resnet.pt', 'decoder.pt', 'params.json'):
        shutil.copy(os.path.join(GOLDEN_DIR, 'eval_cli_chairs', name), xp)
    _check_cli('eval_cli_chairs', xp, tree)


def test_chairs_cli_matches_reference_resnet(tree, tmp_path):
    """The recipe's encoder: the `chairs_resnet` network (ResNet18 + DCGAN decoder) with the det_fill weights the fixture was made with,
    saved by this package's own `save`."""
    xp = write_xp('chairs_resnet', str(tmp_path / 'xp'), os.path.join(GOLDEN_DIR, 'eval_cli_chairs_resnet', 'params.json'))
    _check_cli('eval_cli_chairs_resnet', xp, tree)


# ---------------------------------------------------------------------------------------------------------------------- training
def test_main_trains_on_a_chairs_tree(tree, tmp_path):
    """`main --data chairs --data_dir <tree>` in a fresh process, recorded-graph default: 310 train items in batches of 64 (a ragged last
    batch), finite losses, the four checkpoint files."""
    args = ['--xp_dir', str(tmp_path), '--data_dir', tree, '--device', '0', '--epochs', '1',
            '--batch_size', '64', '--num_workers', '0', '--seed', '3', '--log_interval', '1', '--chkpt_interval', '1',
            '--data', 'chairs', '--architecture', 'resnet', '--decoder_architecture', 'dcgan', '--nt_cond', '2', '--nt_pred', '2', '--offset', '2',
            '--dec_hidden_size', '8', '--res_hidden_size', '16', '--code_size_s', '12', '--code_size_t', '6', '--lamb_ae', '1', '--lamb_s', '1',
            '--precision', 'bf16']
    check_training_run(run_module('main', args, timeout=900), tmp_path, min_losses=5)

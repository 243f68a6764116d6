"""GPU: the TaxiBJ data path -- vs_gather_timeline (csrc/vs_data.hip), data/taxibj.py, `main --data taxibj` on a tree of year files -- and
the evaluation CLI (test/taxibj/test.py) against the reference's own items and per-window MSE on the same inputs (tests/golden/taxibj,
written by tests/make_golden_taxibj.py from the synthetic years of tests/taxibj_inputs.py)."""
import json
import os

import numpy as np
import pytest
import torch

import taxibj_inputs as I
from cli_util import check_training_run, close, run_module, write_xp

pytestmark = pytest.mark.gpu
F = 40                                                   # frames of the kernel tests' timeline


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return I.write_tree(str(tmp_path_factory.mktemp('taxibj')))


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(I.GOLDEN, 'dataset.npz')) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------------------------ the kernel
def _timeline(frame_elems, seed=0):
    """fp32 [F, frame_elems] without a zero value: a zeroed row is recognisable."""
    return np.random.RandomState(1000 + frame_elems + seed).uniform(0.5, 2.0, size=(F, frame_elems)).astype(np.float32)


def _table(seq_len, step):
    """Windows valid for `step`; entries 0 and 1 touch frame 0 and frame F - 1 -- as first and as last frame of a window."""
    if step == 1:
        return np.array([0, F - seq_len, 5, 17, 11, max(F - seq_len - 1, 0), 1, 20], dtype=np.int32)
    return np.array([F - 1, seq_len - 1, 17, 30, seq_len, F - 2, 12, 25], dtype=np.int32)


def _numpy_gather(frames, first, items, seq_len, step):
    rows = first[items].astype(np.int64)[:, None] + step * np.arange(seq_len)[None]
    return frames[rows]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('step', [1, -1])
@pytest.mark.parametrize('rows', [1, 7])
@pytest.mark.parametrize('seq_len', [1, 8])
@pytest.mark.parametrize('frame_elems', [2048, 12, 6])
def test_gather_timeline_matches_numpy(frame_elems, seq_len, rows, step, dtype):
    from spatiotemporal_variable_separation_amd import ops
    frames, first = _timeline(frame_elems), _table(seq_len, step)
    f, t = torch.from_numpy(frames).cuda(), torch.from_numpy(first).cuda()
    for items in ([[0], [1], [4]] if rows == 1 else [[0, 1, 5, 3, 2, 7, 1]]):
        items = np.array(items, dtype=np.int32)
        ref = torch.from_numpy(_numpy_gather(frames, first, items, seq_len, step))
        out = ops.gather_timeline(f, t, torch.from_numpy(items).cuda(), seq_len, step, dtype)
        assert out.dtype == dtype and tuple(out.shape) == (rows, seq_len, frame_elems)
        assert torch.equal(out.cpu(), ref.to(dtype))     # fp32: bit-identical; 16-bit: torch's cast of the fp32 result
        if dtype == torch.float32:
            assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.numpy().view(np.uint32))


@pytest.mark.parametrize('frame_elems', [2048, 6])
@pytest.mark.parametrize('step', [1, -1])
def test_gather_timeline_flags_bad_rows(frame_elems, step):
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd._lib import VarsepHipError
    seq_len = 8
    frames, good_first = _timeline(frame_elems, seed=7), _table(seq_len, step)
    f = torch.from_numpy(frames).cuda()
    good_items = np.array([2, 0, 1, 3], dtype=np.int32)
    past_end, past_start = ((F - seq_len + 1, -1) if step == 1 else (F, seq_len - 2))
    # (bad row, item index or None, table entry of that row's window or None)
    cases = [(1, -1, None), (2, len(good_first), None), (0, 2 ** 31 - 1, None), (3, None, past_end), (1, None, past_start),
             (2, None, 2 ** 31 - 1), (0, None, -(2 ** 31))]
    for row, item, entry in cases:
        items, first = good_items.copy(), good_first.copy()
        if item is not None:
            items[row] = item
        else:
            items[row] = 6                               # a window no other row uses
            first[6] = entry
        t, i = torch.from_numpy(first).cuda(), torch.from_numpy(items).cuda()
        with pytest.raises(VarsepHipError, match='gather_timeline'):
            ops.gather_timeline(f, t, i, seq_len, step)
        ref = torch.from_numpy(_numpy_gather(frames, good_first, good_items, seq_len, step))
        keep = [r for r in range(4) if r != row]
        for dtype in (torch.float32, torch.bfloat16):
            out = ops.gather_timeline(f, t, i, seq_len, step, dtype, validate=False).cpu()
            assert torch.count_nonzero(out[row]) == 0, (row, item, entry)
            assert torch.equal(out[keep], ref.to(dtype)[keep]), (row, item, entry)
    t, i = torch.from_numpy(good_first).cuda(), torch.from_numpy(good_items).cuda()
    with pytest.raises(VarsepHipError):
        ops.gather_timeline(torch.from_numpy(frames), t, i, seq_len, step)
    with pytest.raises(VarsepHipError):
        ops.gather_timeline(f, t.long(), i, seq_len, step)
    with pytest.raises(VarsepHipError):
        ops.gather_timeline(f, t, i.long(), seq_len, step)
    with pytest.raises(VarsepHipError):
        ops.gather_timeline(f.double(), t, i, seq_len, step)


def test_gather_timeline_argument_checks():
    """Every argument-check path of the C entry point returns non-zero with the function's name in the message and launches nothing."""
    from spatiotemporal_variable_separation_amd import _lib, ops
    lib = _lib.load_library()
    f = torch.full((6, 8), 3.0).cuda()
    first = torch.tensor([0, 1, 2], dtype=torch.int32).cuda()
    item = torch.tensor([2, 0], dtype=torch.int32).cuda()
    out = torch.full((2, 2, 8), 7.0).cuda()
    good = dict(frames=f.data_ptr(), n_frames=6, fe=8, first=first.data_ptr(), n_windows=3, step=1, item=item.data_ptr(), rows=2, seq_len=2,
                out=out.data_ptr(), dtype=_lib.F32)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vs_gather_timeline(a['frames'], a['n_frames'], a['fe'], a['first'], a['n_windows'], a['step'], a['item'], a['rows'],
                                      a['seq_len'], a['out'], a['dtype'], None, _lib.stream_ptr())

    cases = [dict(frames=None), dict(first=None), dict(item=None), dict(out=None), dict(n_frames=0), dict(n_frames=-1), dict(fe=0), dict(fe=-4),
             dict(n_windows=0), dict(n_windows=-2), dict(rows=0), dict(rows=-1), dict(rows=65536), dict(seq_len=0), dict(seq_len=-3),
             dict(step=0), dict(step=2), dict(step=-2), dict(dtype=3), dict(dtype=-1)]
    for kw in cases:
        assert call(**kw) != 0, kw
        assert b'vs_gather_timeline' in lib.vs_last_error(), kw
    torch.cuda.synchronize()
    assert torch.all(out == 7.0)                         # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.all(out == 3.0)
    with pytest.raises(_lib.VarsepHipError):
        ops.gather_timeline(f, first, item, 0, 1)
    with pytest.raises(_lib.VarsepHipError):
        ops.gather_timeline(f, first, item, 2, 1, torch.float64)
    with pytest.raises(_lib.VarsepHipError):
        ops.gather_timeline(f, first, item, 2, 3)


# ----------------------------------------------------------------------------------------------------------------- the dataset
@pytest.mark.parametrize('call', sorted(I.CALLS))
def test_every_item_matches_the_reference(tree, golden, call):
    from spatiotemporal_variable_separation_amd._lib import VarsepHipError
    from spatiotemporal_variable_separation_amd.data.taxibj import TaxiBJ
    kw = I.CALLS[call]
    L, nc = kw['len_closeness'], kw['nt_cond']
    halves = dict(zip(('train', 'test'), TaxiBJ.make_datasets(tree, device='cuda', **kw)))
    assert [len(halves['train']), len(halves['test'])] == golden['len_%s' % call].tolist()
    assert halves['train'].frames is halves['test'].frames and halves['train'].frames.dtype == torch.float32
    assert halves['train'].mmn is halves['test'].mmn
    assert float(halves['test'].mmn._min) == float(golden['min_%s' % call]) and float(halves['test'].mmn._max) == float(golden['max_%s' % call])
    for half, ds in halves.items():
        assert ds.device_resident and ds.first.dtype == torch.int32 and ds.first.is_cuda
        crcs = []
        for lo in range(0, len(ds), 256):
            cond, target = ds.batch(list(range(lo, min(lo + 256, len(ds)))))
            assert tuple(cond.shape[1:]) == (nc, 2, 32, 32) and tuple(target.shape[1:]) == (L - nc, 2, 32, 32)
            crcs.append(I.item_crcs(torch.cat([cond, target], dim=1).cpu().numpy()))
        assert np.array_equal(np.concatenate(crcs), golden['crc_%s_%s' % (call, half)]), (call, half)
    for c, half, index in I.WHOLE_ITEMS:
        if c != call:
            continue
        ds, want = halves[half], golden[I.whole_item_key(c, half, index)]
        i = index % len(ds)
        cond, target = ds[i]
        got = torch.cat([cond, target]).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (c, half, index)
        cb, tb = ds.batch([i])
        assert torch.equal(cb[0], cond) and torch.equal(tb[0], target)
        on_device = ds.batch(torch.tensor([i], dtype=torch.int32).cuda())          # a device index tensor goes to the kernel as it is
        assert torch.equal(on_device[0][0], cond) and torch.equal(on_device[1][0], target)
    ds = halves['test']
    idx = [0, len(ds) - 1, len(ds) // 2, 3]
    cond, target = ds.batch(idx)
    c16, t16 = ds.batch(idx, torch.bfloat16)
    assert c16.dtype == torch.bfloat16 and torch.equal(c16, cond.to(torch.bfloat16)) and torch.equal(t16, target.to(torch.bfloat16))
    for bad in ([len(ds)], [0, -1], []):
        with pytest.raises(IndexError):
            ds.batch(bad)
    with pytest.raises(VarsepHipError):
        ds.batch(torch.tensor([len(ds)], dtype=torch.int32).cuda())
    with pytest.raises(VarsepHipError):
        TaxiBJ.make_datasets(tree, device='cpu', **kw)


def test_device_loader_visits_the_dataloader_items(tree):
    """DeviceBatchLoader(TaxiBJ) under a fixed torch.manual_seed yields the items `DataLoader(shuffle=True)` would: a DataLoader iterator
    draws its base seed, then its RandomSampler draws the permutation."""
    from torch.utils.data import BatchSampler, RandomSampler
    from spatiotemporal_variable_separation_amd.data.taxibj import TaxiBJ, build_windows
    from spatiotemporal_variable_separation_amd.data.device import DeviceBatchLoader
    frames, first, n_train, _ = build_windows(tree, len_closeness=8)
    ds = TaxiBJ.make_datasets(tree, len_closeness=8, nt_cond=4, device='cuda')[0]
    assert len(ds) == n_train == 192
    torch.manual_seed(17)
    torch.empty((), dtype=torch.int64).random_()          # _BaseDataLoaderIter.__init__: the base seed
    want = list(BatchSampler(RandomSampler(ds), 50, False))
    assert sorted(i for b in want for i in b) == list(range(192)) and len(want[-1]) == 192 % 50
    torch.manual_seed(17)
    got = list(DeviceBatchLoader(ds, 50, shuffle=True))
    assert len(got) == len(want)
    for (cond, target), items in zip(got, want):
        assert cond.shape[0] == len(items)
        ref = I.assemble(frames, first, items, 8)
        assert np.array_equal(cond.cpu().numpy(), ref[:, :4]) and np.array_equal(target.cpu().numpy(), ref[:, 4:])


# --------------------------------------------------------------------------------------------------------------------- the CLI
@pytest.fixture(scope='module')
def xp(tmp_path_factory):
    """The `vgg32_tiny` network with the det_fill weights the fixture was made with, saved by this package's own `save`."""
    return write_xp('vgg32_tiny', str(tmp_path_factory.mktemp('taxibj_xp')), os.path.join(I.GOLDEN, 'eval_cli', 'params.json'))


def test_taxibj_cli_prints_the_reference_mse(tree, xp):
    stdout = run_module('test.taxibj.test', ['--xp_dir', xp, '--data_dir', tree, '--batch_size', '200', '--device', '0', '--precision', 'fp32'])
    lines = [q for q in stdout.splitlines() if q.startswith('MSE at t+4:')]
    assert len(lines) == 1, stdout[-2000:]
    got = float(lines[0].split(':', 1)[1])
    with open(os.path.join(I.GOLDEN, 'eval_cli', 'printed.json')) as f:
        want = json.load(f)['mse_t4']
    print('printed', got, 'reference', want)
    assert close(got, want), (got, want)


def test_taxibj_mse_array_matches_reference(tree, xp):
    """Per-window, per-frame MSE [1344, 4] through the CLI's own load_dataset / compute_mse, in ragged batches of 200."""
    from spatiotemporal_variable_separation_amd.test.taxibj import test as cli
    from spatiotemporal_variable_separation_amd.test.utils import load_model
    from spatiotemporal_variable_separation_amd.utils.helper import load_json
    cfg = load_json(os.path.join(xp, 'params.json'))
    cfg.device, cfg.data_dir, cfg.xp_dir, cfg.nt_pred = torch.device('cuda', 0), tree, xp, 4
    test_set = cli.load_dataset(cfg)
    try:
        mse = np.concatenate(cli.compute_mse(cfg, 200, test_set, load_model(cfg)), axis=0)
    finally:
        torch.set_grad_enabled(True)
    with np.load(os.path.join(I.GOLDEN, 'eval_cli', 'mse.npz')) as z:
        want = z['mse']
    assert len(test_set) == I.N_TEST and mse.shape == want.shape == (I.N_TEST, 4)
    print('max relative difference', float(np.abs(mse / want - 1).max()), 'smallest reference value', float(want.min()))
    assert close(mse, want), np.abs(mse / want - 1).max()


# ---------------------------------------------------------------------------------------------------------------------- training
def test_main_trains_on_a_taxibj_tree(tree, tmp_path):
    """`main --data taxibj --data_dir <tree>` in a fresh process, recorded-graph default: with 2 + 2 frames per item the train half holds
    212 windows, in batches of 64 (a ragged last batch of 20); finite losses, the four checkpoint files."""
    args = ['--xp_dir', str(tmp_path), '--data_dir', tree, '--device', '0', '--epochs', '1',
            '--batch_size', '64', '--num_workers', '0', '--seed', '3', '--log_interval', '1', '--chkpt_interval', '1',
            '--data', 'taxibj', '--architecture', 'vgg', '--nt_cond', '2', '--nt_pred', '2', '--offset', '2', '--enc_hidden_size', '8',
            '--dec_hidden_size', '8', '--res_hidden_size', '16', '--code_size_s', '12', '--code_size_t', '6', '--precision', 'bf16']
    check_training_run(run_module('main', args), tmp_path, min_losses=4)

"""GPU: the SST data path (data/sst.py on vs_gather_timeline, `main --data sst` on a tree of zone files), the fused evaluation metrics
(vs_sst_frame_metrics, csrc/vs_eval.hip) against an fp64 statement of test/sst/test.py:57-71, and the evaluation CLI (test/sst/test.py)
against the reference's own items and per-window arrays on the same inputs (tests/golden/sst, written by tests/make_golden_sst.py from the
synthetic zones of tests/sst_inputs.py)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sst_inputs as I
from cli_util import PKG, ROOT, check_training_run, close, write_xp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return I.write_tree(str(tmp_path_factory.mktemp('sst')))


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(I.GOLDEN, 'dataset.npz')) as z:
        return {k: z[k] for k in z.files}


# ----------------------------------------------------------------------------------------------------------------- the dataset
@pytest.mark.parametrize('call', sorted(I.CALLS))
def test_every_item_matches_the_reference(tree, golden, call):
    from spatiotemporal_variable_separation_amd._lib import VarsepHipError
    from spatiotemporal_variable_separation_amd.data.sst import SST
    kw = I.CALLS[call]
    nc, npred = kw['nt_cond'], kw['nt_pred']
    ds = SST(tree, nc, npred, kw['train'], zones=kw['zones'], eval=True, device='cuda')
    assert len(ds) == int(golden['len_%s' % call]) and ds.device_resident
    assert ds.frames.dtype == torch.float32 and ds.frames.is_cuda and ds.consts.is_cuda and ds.zone_range.is_cuda
    assert ds.first.dtype == torch.int32 and ds.first.is_cuda
    want_crc, want_const, want_id = golden['crc_%s' % call], golden['const_%s' % call], golden['file_id_%s' % call]
    consts = ds.consts.cpu().numpy()
    everything = {}
    for how in ('list', 'tensor'):
        parts = []
        for lo in range(0, len(ds), 100):
            items = list(range(lo, min(lo + 100, len(ds))))
            idx = items if how == 'list' else torch.tensor(items, dtype=torch.int32).cuda()
            cond, target, day0, zone = ds.batch(idx)
            assert tuple(cond.shape[1:]) == (nc, 1, 64, 64) and tuple(target.shape[1:]) == (npred, 1, 64, 64)
            assert day0.dtype == zone.dtype == torch.int32 and day0.is_cuda and zone.is_cuda
            parts.append(torch.cat([cond, target], dim=1))
            d0 = day0.cpu().numpy().astype(np.int64)
            got = consts[d0[:, None] + np.arange(npred)[None]]
            assert np.array_equal(got.view(np.uint32), want_const[items].view(np.uint32)), (call, how, lo)
            assert np.array_equal(np.asarray(kw['zones'])[zone.cpu().numpy()], want_id[items]), (call, how, lo)
        everything[how] = torch.cat(parts)
        assert np.array_equal(I.item_crcs(everything[how].cpu().numpy()), want_crc), (call, how)
    full = everything['list']
    for c, index in I.WHOLE_ITEMS:
        if c == call:
            want = golden[I.whole_item_key(c, index)]
            assert np.array_equal(full[index].cpu().numpy().view(np.uint32), want.view(np.uint32)), (c, index)
            item = ds[index % len(ds)]
            assert len(item) == 7 and torch.equal(torch.cat(item[:2]), full[index]) and item[6] == int(want_id[index])
            for got, k in zip(item[2:6], (2, 3, 0, 1)):                      # mu_clim, std_clim, mu_norm, std_norm
                assert tuple(got.shape) == (npred, 1, 1) and np.array_equal(got.cpu().numpy().reshape(-1), want_const[index][:, k])
    assert np.array_equal(ds.zone_range.cpu().numpy(), golden['range_%s' % call].astype(np.float32))
    # 16-bit batches are the round-to-nearest cast of the fp32 items; without eval a batch is (cond, target)
    plain = SST(tree, nc, npred, kw['train'], zones=kw['zones'], device='cuda')
    idx = [0, len(ds) - 1, len(ds) // 2, 3]
    for dtype in (torch.bfloat16, torch.float16):
        for index in (idx, torch.tensor(idx, dtype=torch.int32).cuda()):
            out = plain.batch(index, dtype)
            assert len(out) == 2 and out[0].dtype == dtype
            assert torch.equal(torch.cat(out, dim=1), full[idx].to(dtype))
    cond, target = plain[idx[1]]
    assert torch.equal(torch.cat([cond, target]), full[idx[1]])
    for bad in ([len(ds)], [0, -1], []):
        with pytest.raises(IndexError):
            ds.batch(bad)
    with pytest.raises(VarsepHipError):
        ds.batch(torch.tensor([len(ds)], dtype=torch.int32).cuda())
    with pytest.raises(VarsepHipError):
        SST(tree, nc, npred, kw['train'], zones=kw['zones'], device='cpu')


def test_device_loader_serves_a_ragged_last_batch(tree, golden):
    from spatiotemporal_variable_separation_amd.data.sst import SST
    from spatiotemporal_variable_separation_amd.data.device import DeviceBatchLoader
    kw = I.CALLS['test']
    ds = SST(tree, kw['nt_cond'], kw['nt_pred'], False, zones=kw['zones'], eval=True, device='cuda')
    batches = list(DeviceBatchLoader(ds, 16, shuffle=False))
    assert [b[0].shape[0] for b in batches] == [16, 16, 12] and all(len(b) == 4 for b in batches)
    items = torch.cat([torch.cat(b[:2], dim=1) for b in batches])
    assert np.array_equal(I.item_crcs(items.cpu().numpy()), golden['crc_test'])
    assert torch.cat([b[3] for b in batches]).cpu().tolist() == [i // 11 for i in range(44)]


# ------------------------------------------------------------------------------------------------------------------ the kernel
SHAPES = [(11, 11), (12, 17), (64, 64)]
N_ZONES = 3


@functools.lru_cache(maxsize=None)
def _case(H, W, T, rows):
    """Inputs on the device, the fp64 values of both outputs (sst_inputs.metrics_fp64), and the fp32 composition of existing ops --
    torch broadcasting plus ops.frame_metrics -- with its largest SSIM error against fp64.  Computed once per case and shared.
    Smooth targets plus noisy forecasts; the constants include negative mu_norm / mu_clim, and zone 0's min is negative."""
    from spatiotemporal_variable_separation_amd import ops
    g = torch.Generator().manual_seed(1000 * H + 100 * W + 10 * T + rows)
    yy, xx = torch.meshgrid(torch.arange(H) / 16.0, torch.arange(W) / 16.0, indexing='ij')
    phase = torch.rand((rows, T, 1, 1), generator=g) * 6.28
    target = 1.2 * torch.sin(2.1 * xx + 1.3 * yy + phase) + 0.4 * torch.randn((rows, T, H, W), generator=g)
    pred = target + 0.5 * torch.randn((rows, T, H, W), generator=g)
    n_days = T + 7
    consts = torch.stack([torch.rand(n_days, generator=g) - 0.6, 0.5 + torch.rand(n_days, generator=g),
                          3 * torch.rand(n_days, generator=g) - 1.0, 0.6 + 0.8 * torch.rand(n_days, generator=g)], dim=1)
    consts[0, 0], consts[1, 2] = -0.55, -0.9
    zone_range = torch.tensor([[-3.25, 3.5], [0.5, 4.75], [-4.0, -0.5]])
    day0 = torch.randint(0, n_days - T + 1, (rows,), generator=g).to(torch.int32)
    day0[0] = 0
    day0[-1] = n_days - T                                 # the last row ends on the last day of `consts`
    zone = (torch.arange(rows) % N_ZONES).to(torch.int32)
    dev = [a.cuda() for a in (pred, target, consts, day0, zone, zone_range)]
    pred, target, consts, day0, zone, zone_range = dev
    per_row = consts[day0.long()[:, None] + torch.arange(T, device='cuda')[None]]            # [rows, T, 4]
    lo, hi = zone_range[zone.long(), 0], zone_range[zone.long(), 1]
    mse64, ssim64 = I.metrics_fp64(pred, target, per_row, lo, hi)
    # the unfused composition, in fp32 as the script evaluates it
    mn, sn, mc, sc = (per_row[:, None, :, k, None, None] for k in range(4))
    p = ((pred[:, :, None] * sn) + mn) * sc + mc
    t = ((target[:, :, None] * sn) + mn) * sc + mc
    mse_u = (p - t).pow(2).mean(dim=-1).mean(dim=-1).mean(dim=-1)
    lo5, hi5 = lo.view(-1, 1, 1, 1, 1), hi.view(-1, 1, 1, 1, 1)
    _, ssim_u = ops.frame_metrics((p - lo5) / (hi5 - lo5), (t - lo5) / (hi5 - lo5), max_val=1.0)
    e_unfused = float((ssim_u.double() - ssim64).abs().max())
    return dict(dev=dev, mse64=mse64.cpu().numpy(), ssim64=ssim64.cpu().numpy(), mse_u=mse_u.cpu().numpy(), ssim_u=ssim_u.cpu().numpy(),
                e_unfused=e_unfused)


@pytest.mark.parametrize('rows', [1, 5])
@pytest.mark.parametrize('T', [1, 3, 10])
@pytest.mark.parametrize('shape', SHAPES)
def test_sst_frame_metrics_matches_fp64(shape, T, rows):
    """MSE: the project's rule |a - b| <= 1e-3 |b| + 1e-5.  SSIM: |a - b| <= 1e-3 |b| + 4 E_unfused, where E_unfused is the largest error,
    on the same inputs, of the unfused fp32 composition (torch broadcasting + ops.frame_metrics) against the same fp64 values: an
    independent fp32 implementation of the same formula, so 4x covers another summation order and FMA contraction, no more."""
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd.utils.metrics import sst_metrics
    c = _case(shape[0], shape[1], T, rows)
    pred, target, consts, day0, zone, zone_range = c['dev']
    mse, ssim = ops.sst_frame_metrics(pred, target, consts, day0, zone, zone_range)
    assert mse.dtype == ssim.dtype == torch.float32 and tuple(mse.shape) == (rows, T) and tuple(ssim.shape) == (rows, T, T)
    mse, ssim = mse.cpu().numpy(), ssim.cpu().numpy()
    e_fused = float(np.abs(ssim - c['ssim64']).max())
    print('H x W', shape, 'T', T, 'rows', rows, 'E_unfused', c['e_unfused'], 'E_fused', e_fused, 'largest relative MSE error',
          float(np.abs(mse / c['mse64'] - 1).max()), 'SSIM from', float(c['ssim64'].min()), 'to', float(c['ssim64'].max()))
    assert np.isfinite(c['ssim64']).all() and c['e_unfused'] > 0 and close(c['mse_u'], c['mse64'], floor=1e-5)      # the yardstick itself
    assert close(mse, c['mse64'], floor=1e-5)
    assert close(ssim, c['ssim64'], floor=4 * c['e_unfused'])
    m5, s5 = sst_metrics(pred[:, :, None], target[:, :, None], consts, day0, zone, zone_range)               # [B, T, 1, H, W] frames
    assert np.array_equal(m5.cpu().numpy(), mse) and np.array_equal(s5.cpu().numpy(), ssim)


def test_sst_frame_metrics_sixteen_days():
    """T = 16, the largest window the kernel takes, on 64 x 64 planes; T = 17 is refused."""
    from spatiotemporal_variable_separation_amd import _lib, ops
    c = _case(64, 64, 16, 2)
    pred, target, consts, day0, zone, zone_range = c['dev']
    mse, ssim = ops.sst_frame_metrics(pred, target, consts, day0, zone, zone_range)
    assert close(mse.cpu().numpy(), c['mse64'], floor=1e-5) and close(ssim.cpu().numpy(), c['ssim64'], floor=4 * c['e_unfused'])
    big = torch.zeros((1, 17, 11, 11)).cuda()
    with pytest.raises(_lib.VarsepHipError, match='vs_sst_frame_metrics'):
        ops.sst_frame_metrics(big, big, torch.ones((20, 4)).cuda(), day0[:1], zone[:1], zone_range)


def test_sst_frame_metrics_flags_bad_rows():
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd._lib import VarsepHipError
    T, rows = 3, 5
    c = _case(12, 17, T, rows)
    pred, target, consts, day0, zone, zone_range = c['dev']
    n_days = consts.shape[0]
    for row, which, value in [(1, 'day0', -1), (4, 'day0', n_days - T + 1), (0, 'day0', 2 ** 31 - 1), (2, 'day0', -(2 ** 31)),
                              (3, 'zone', -1), (0, 'zone', N_ZONES), (2, 'zone', 2 ** 31 - 1)]:
        d, z = day0.clone(), zone.clone()
        (d if which == 'day0' else z)[row] = value
        with pytest.raises(VarsepHipError, match='sst_frame_metrics'):
            ops.sst_frame_metrics(pred, target, consts, d, z, zone_range)
        mse, ssim = ops.sst_frame_metrics(pred, target, consts, d, z, zone_range, validate=False)
        mse, ssim = mse.cpu().numpy(), ssim.cpu().numpy()
        keep = [r for r in range(rows) if r != row]
        assert not mse[row].any() and not ssim[row].any(), (row, which, value)
        assert close(mse[keep], c['mse64'][keep], floor=1e-5) and close(ssim[keep], c['ssim64'][keep], floor=4 * c['e_unfused']), (row, which, value)
    for bad in [dict(pred=pred.cpu()), dict(pred=pred.double()), dict(pred=pred[:, :2]), dict(consts=consts[:, :3].contiguous()),
                dict(day0=day0.long()), dict(zone=zone[:2]), dict(zone_range=zone_range.double()), dict(zone=zone.long())]:
        a = dict(pred=pred, target=target, consts=consts, day0=day0, zone=zone, zone_range=zone_range)
        a.update(bad)
        with pytest.raises(VarsepHipError):
            ops.sst_frame_metrics(**a)


def test_sst_frame_metrics_argument_checks():
    """Every argument-check path of the C entry point returns non-zero with the function's name in the message and launches nothing."""
    from spatiotemporal_variable_separation_amd import _lib
    lib = _lib.load_library()
    rows, T, H, W = 2, 2, 11, 12
    pred, target = torch.rand((rows, T, H, W)).cuda(), torch.rand((rows, T, H, W)).cuda()
    consts = torch.tensor([[0.0, 1.0, 0.0, 1.0]] * 4).cuda()
    day0, zone = torch.tensor([0, 2], dtype=torch.int32).cuda(), torch.zeros(2, dtype=torch.int32).cuda()
    zone_range = torch.tensor([[0.0, 1.0]]).cuda()
    mse, ssim = torch.full((rows, T), 7.0).cuda(), torch.full((rows, T, T), 7.0).cuda()
    bad = torch.zeros(1, dtype=torch.int32).cuda()
    good = dict(pred=pred.data_ptr(), target=target.data_ptr(), rows=rows, T=T, H=H, W=W, consts=consts.data_ptr(), n_days=4, day0=day0.data_ptr(),
                zone=zone.data_ptr(), zone_range=zone_range.data_ptr(), n_zones=1, k1=0.01, k2=0.03, sigma=1.5, mse=mse.data_ptr(),
                ssim=ssim.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.vs_sst_frame_metrics(a['pred'], a['target'], a['rows'], a['T'], a['H'], a['W'], a['consts'], a['n_days'], a['day0'], a['zone'],
                                        a['zone_range'], a['n_zones'], a['k1'], a['k2'], a['sigma'], a['mse'], a['ssim'], bad.data_ptr(),
                                        _lib.stream_ptr())

    cases = [dict(pred=None), dict(target=None), dict(consts=None), dict(day0=None), dict(zone=None), dict(zone_range=None),
             dict(mse=None, ssim=None), dict(rows=0), dict(rows=-1), dict(rows=2 ** 31), dict(T=0), dict(T=-1), dict(T=17), dict(H=10), dict(W=10),
             dict(H=-64), dict(n_days=0), dict(n_days=-3), dict(n_zones=0), dict(n_zones=-1), dict(sigma=0.0), dict(sigma=-1.5),
             dict(H=200, W=200)]
    for kw in cases:
        assert call(**kw) != 0, kw
        assert b'vs_sst_frame_metrics' in lib.vs_last_error(), kw
    torch.cuda.synchronize()
    assert torch.all(mse == 7.0) and torch.all(ssim == 7.0) and int(bad.item()) == 0           # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    # identity constants and range (0, 1): the plain frame metrics of the planes, for every day
    from spatiotemporal_variable_separation_amd import ops
    m, s = ops.frame_metrics(pred, target, max_val=1.0)
    assert int(bad.item()) == 0 and close(mse.cpu().numpy(), m.cpu().numpy(), floor=1e-5)
    assert close(ssim.cpu().numpy(), s[:, :, None].expand(rows, T, T).cpu().numpy(), floor=1e-5)
    # either output alone
    mse.fill_(7.0)
    assert call(ssim=None) == 0 and call(mse=None) == 0
    torch.cuda.synchronize()
    assert close(mse.cpu().numpy(), m.cpu().numpy(), floor=1e-5)


# --------------------------------------------------------------------------------------------------------------------- the CLI
@pytest.fixture(scope='module')
def xp(tmp_path_factory):
    """The `sst_skip` network with the det_fill weights the fixture was made with, saved by this package's own `save`."""
    return write_xp('sst_skip', str(tmp_path_factory.mktemp('sst_xp')), os.path.join(I.GOLDEN, 'eval_cli', 'params.json'))


RUN_CLI = ('import sys, numpy as np\n'
           'from %s.test.sst import test as cli\n'
           'out = sys.argv.pop(1)\n'
           'mse, ssim = cli.main(cli.build_parser().parse_args(sys.argv[1:]))\n'
           'np.savez(out, mse=mse, ssim=ssim)\n' % PKG)


@pytest.fixture(scope='module')
def cli_runs(tree, xp, tmp_path_factory):
    """{batch size: (stdout, mse, ssim)} of the CLI's `main` in a fresh process each, on the .npz tree: 16 leaves a ragged last batch of
    12, 1 is the reference's one window at a time."""
    out_dir = tmp_path_factory.mktemp('sst_cli')
    runs = {}
    for batch_size in (16, 1):
        out = str(out_dir / ('b%d.npz' % batch_size))
        r = subprocess.run([sys.executable, '-c', RUN_CLI, out, '--xp_dir', xp, '--data_dir', tree, '--batch_size', str(batch_size),
                            '--device', '0', '--precision', 'fp32'], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        with np.load(out) as z:
            runs[batch_size] = (r.stdout, z['mse'], z['ssim'])
    return runs


@pytest.fixture(scope='module')
def reference_metrics():
    with np.load(os.path.join(I.GOLDEN, 'eval_cli', 'metrics.npz')) as z:
        metrics = {k: z[k] for k in z.files}
    with open(os.path.join(I.GOLDEN, 'eval_cli', 'printed.json')) as f:
        return metrics, json.load(f)


@pytest.mark.parametrize('batch_size', [16, 1])
def test_sst_cli_arrays_match_the_reference(cli_runs, reference_metrics, batch_size):
    """MSE [44, 10] by the project's rule; SSIM [44, 10, 10] by |a - b| <= 1e-3 |b| + 4 E, E = the reference's own largest distance from the
    fp64 statement of its formula (printed.json)."""
    metrics, printed = reference_metrics
    _, mse, ssim = cli_runs[batch_size]
    assert mse.shape == (I.N_TEST, 10) and ssim.shape == (I.N_TEST, 10, 10) and 0 < printed['E'] <= 1e-4
    print('batch', batch_size, 'largest relative MSE difference', float(np.abs(mse / metrics['mse'] - 1).max()), 'largest SSIM difference',
          float(np.abs(ssim - metrics['ssim']).max()), 'to fp64', float(np.abs(ssim - metrics['ssim_fp64']).max()), 'E', printed['E'])
    assert close(mse, metrics['mse'], floor=1e-5)
    assert close(ssim, metrics['ssim'], floor=4 * printed['E'])


def test_sst_cli_batch_sizes_agree(cli_runs, reference_metrics):
    E = reference_metrics[1]['E']
    assert close(cli_runs[1][1], cli_runs[16][1], floor=1e-5) and close(cli_runs[1][2], cli_runs[16][2], floor=4 * E)


def test_sst_cli_prints_the_reference_lines(cli_runs, reference_metrics):
    printed = reference_metrics[1]
    stdout = cli_runs[16][0]
    for head, key in (('MSE at t+10', 'mse_t10'), ('MSE at t+6', 'mse_t6'), ('SSIM at t+10', 'ssim_t10'), ('SSIM at t+6', 'ssim_t6')):
        lines = [q for q in stdout.splitlines() if q.startswith(head + ':')]
        assert len(lines) == 1, stdout[-2000:]
        got = float(lines[0].split(':', 1)[1])
        print(head, got, 'reference', printed[key])
        assert abs(got - printed[key]) <= 1e-3 * abs(printed[key]), (head, got, printed[key])
    mse, ssim = cli_runs[16][1], cli_runs[16][2]
    line = [q for q in stdout.splitlines() if q.startswith('SSIM at t+6:')][0]
    assert abs(float(line.split(':', 1)[1]) - float(np.mean(ssim.mean(axis=0)[:6]))) <= 1e-6       # the mean over all (t < 6, c) pairs


# ---------------------------------------------------------------------------------------------------------------------- training
def test_main_trains_on_an_sst_tree(tmp_path):
    """`main --data sst --data_dir <tree> --zones 1 2 17` in a fresh process, recorded-graph default: three zones of 30 days hold
    3 x (24 - 2 - 2 - 1) = 57 train windows, two steps in batches of 32 (a ragged last batch of 25); finite losses, the checkpoint files."""
    short = {zone: {k: v[:30] for k, v in z.items()} for zone, z in I.arrays().items()}
    data_dir = I.write_tree(str(tmp_path / 'zones'), zones=(1, 2, 17), zone_arrays=short)
    xp_dir = tmp_path / 'xp'
    cmd = [sys.executable, '-m', '%s.main' % PKG, '--xp_dir', str(xp_dir), '--data_dir', data_dir, '--device', '0', '--epochs', '1',
           '--batch_size', '32', '--num_workers', '0', '--seed', '3', '--log_interval', '1', '--chkpt_interval', '1',
           '--data', 'sst', '--zones', '1', '2', '17', '--architecture', 'encoderSST', '--decoder_architecture', 'decoderSST', '--skipco',
           '--nt_cond', '2', '--nt_pred', '2', '--offset', '0', '--n_blocks', '2', '--res_hidden_size', '16', '--code_size_s', '12',
           '--code_size_t', '8', '--lamb_ae', '1', '--lamb_s', '100', '--lamb_t', '5e-6', '--precision', 'bf16']
    r = subprocess.run(['timeout', '-k', '10', '300'] + cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    check_training_run(r.stdout, xp_dir, min_losses=2)

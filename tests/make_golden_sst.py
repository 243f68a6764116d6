"""Generate tests/golden/sst/ by running the REFERENCE's SST loader (var_sep.data.sst.SST) and evaluation script (var_sep.test.sst.test --
its own `compute_mse_ssim` and `main`, on the CPU) on the synthetic zones of tests/sst_inputs.py.

TEST INFRASTRUCTURE ONLY; runs only where the reference is available (VARSEP_REFERENCE, default /root/reference):

    python tests/make_golden_sst.py

The reference reads its files through netCDF4, which need not exist where this runs: sst_inputs.install_fake_netcdf4 puts a stand-in with
`Dataset(fp, 'r').variables[name][:]` (a masked array) into sys.modules, through which the UNMODIFIED reference loader and script run.
`torch.load` reads whole-module pickles, as tests/make_golden_eval_cli.py arranges it.

Written:
  * dataset.npz: for the two calls of sst_inputs.CALLS (both made with eval=True, which adds the constants to the same frames) the length,
    the zlib.crc32 of every item's fp32 bytes (cond then target), the whole items of sst_inputs.WHOLE_ITEMS, the constants of every item
    [n, nt_pred, 4] = (mu_norm, std_norm, mu_clim, std_clim) rounded to fp32 as the script rounds them, the file id of every item and the
    script's per-zone (min, max) as NumPy gives them (float64);
  * eval_cli/: params.json, flags.json, printed.json and metrics.npz (mse [44, 10], ssim [44, 10, 10] of the reference, and ssim_fp64: the
    fp64 statement of the same formula, sst_inputs.metrics_fp64, on the same forecasts) for the `sst_skip` network of
    oracle/golden_configs.py filled with oracle.detdata.det_fill -- NO checkpoint: the test rebuilds the weights with the same det_fill.
    printed.json also holds E, the largest |ssim - ssim_fp64|: the reference's own fp32 error, which bounds the tests' comparison.
Asserted here, on the reference alone: every per-window MSE >= 1e-3 (the absolute term of |a - b| <= 1e-3 |b| + 1e-5 never decides a case),
E <= 1e-4, and |mean SSIM| of both printed lines >= 1e-2.
"""
import ast
import contextlib
import functools
import io
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = os.environ.get('VARSEP_REFERENCE', '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import sst_inputs as I  # noqa: E402
from eval_cli_inputs import write_params  # noqa: E402
from oracle.detdata import det_fill  # noqa: E402
from oracle.golden_configs import CONFIGS  # noqa: E402

SCRIPT = 'var_sep/test/sst/test.py'
FILE_LIMIT = 440 * 1000          # the limit of tests/make_golden_taxibj.py
MSE_FLOOR, E_CEILING, SSIM_FLOOR = 1e-3, 1e-4, 1e-2
PRINTED = {'MSE at t+10': 'mse_t10', 'MSE at t+6': 'mse_t6', 'SSIM at t+10': 'ssim_t10', 'SSIM at t+6': 'ssim_t6'}


def _flags(path):
    """[[flag, default, type, required], ...] of the script's `p.add_argument` calls."""
    out = []
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Call) and getattr(node.func, 'attr', None) == 'add_argument':
            kw = {k.arg: k.value for k in node.keywords}
            default = ast.literal_eval(kw['default']) if 'default' in kw else None
            typ = kw['type'].id if 'type' in kw else None
            req = ast.literal_eval(kw['required']) if 'required' in kw else False
            out.append([ast.literal_eval(node.args[0]), default, typ, req])
    return out


def dataset_fixture(ref_sst, ref_test, data_dir, out):
    z = {}
    for call, kw in I.CALLS.items():
        ds = ref_sst.SST(data_dir, kw['nt_cond'], kw['nt_pred'], kw['train'], zones=kw['zones'], eval=True)
        items, consts, file_ids = [], [], []
        for i in range(len(ds)):
            cond, target, mu_clim, std_clim, mu_norm, std_norm, file_id = ds[i]
            assert cond.dtype == target.dtype == torch.float32 and tuple(cond.shape) == (kw['nt_cond'], 1, 64, 64)
            items.append(torch.cat([cond, target]).numpy())
            consts.append(np.stack([torch.tensor(c, dtype=torch.float).numpy().reshape(-1) for c in (mu_norm, std_norm, mu_clim, std_clim)], axis=1))
            file_ids.append(file_id)
        items = np.stack(items)
        mins, maxs = ref_test.get_min(ds)
        z['len_%s' % call] = np.int64(len(ds))
        z['crc_%s' % call] = I.item_crcs(items)
        z['const_%s' % call] = np.stack(consts).astype(np.float32)
        z['file_id_%s' % call] = np.array(file_ids, dtype=np.int64)
        z['range_%s' % call] = np.array([[mins[q], maxs[q]] for q in kw['zones']], dtype=np.float64)
        for c, index in I.WHOLE_ITEMS:
            if c == call:
                z[I.whole_item_key(c, index)] = items[index]
        print(call, 'length', len(ds), 'zone dtypes', [str(ds.data[q].dtype) for q in kw['zones']], 'range', z['range_%s' % call].tolist())
        assert {str(ds.data[q].dtype) for q in kw['zones']} == {'float32', 'float64'}           # both promotions occur
    path = os.path.join(out, 'dataset.npz')
    np.savez_compressed(path, **z)
    return path


def eval_fixture(ref_test, DotDict, save, data_dir, out):
    from oracle.make_golden import _reference_modules, build_reference
    rf, rm, ru, _ = _reference_modules()
    cfg = CONFIGS['sst_skip']
    assert cfg['nt_cond'] == I.PARAMS['nt_cond'] and cfg['offset'] == I.PARAMS['offset'] and cfg['skipco'] == I.PARAMS['skipco']
    net = det_fill(build_reference(cfg, rf, rm, ru), salt=cfg['salt'])
    os.makedirs(out, exist_ok=True)
    xp = tempfile.mkdtemp(prefix='sst_xp_')
    try:
        save(xp, net)
        write_params(xp, I.PARAMS)
        from var_sep.utils.helper import load_json
        from var_sep.test.utils import load_model
        xp_config = load_json(os.path.join(xp, 'params.json'))
        xp_config.device, xp_config.data_dir, xp_config.xp_dir, xp_config.nt_pred = torch.device('cpu'), data_dir, xp, 10
        test_set = ref_test.load_dataset(xp_config, train=False)
        sep_net = load_model(xp_config, None)
        all_mse, all_ssim = ref_test.compute_mse_ssim(xp_config, test_set, sep_net)
        mse, ssim = np.concatenate(all_mse, axis=0), np.concatenate(all_ssim, axis=0)
        assert mse.shape == (I.N_TEST, 10) and ssim.shape == (I.N_TEST, 10, 10)

        # the fp64 statement of the same formula on the same forecasts
        mins, maxs = ref_test.get_min(test_set)
        preds, targets, consts, lo, hi = [], [], [], [], []
        for cond, target, mu_clim, std_clim, mu_norm, std_norm, file_id in test_set:
            preds.append(sep_net.get_forecast(cond.unsqueeze(0), target.size(0))[0][0, :, 0])
            targets.append(target[:, 0])
            consts.append(np.stack([torch.tensor(c, dtype=torch.float).numpy().reshape(-1) for c in (mu_norm, std_norm, mu_clim, std_clim)], axis=1))
            lo.append(float(mins[file_id]))
            hi.append(float(maxs[file_id]))
        mse64, ssim64 = I.metrics_fp64(torch.stack(preds), torch.stack(targets), np.stack(consts), np.array(lo), np.array(hi))
        mse64, ssim64 = mse64.numpy(), ssim64.numpy()
        torch.set_grad_enabled(True)
        E = float(np.abs(ssim - ssim64).max())

        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
            ref_test.main(DotDict(data_dir=data_dir, xp_dir=xp, epoch=None, device=None))
        torch.set_grad_enabled(True)
        printed = {}
        for line in buf.getvalue().splitlines():
            head = line.split(':', 1)[0]
            if head in PRINTED:
                printed[PRINTED[head]] = float(line.split(':', 1)[1])
        assert sorted(printed) == sorted(PRINTED.values()), buf.getvalue()
        want = {'mse_t10': np.mean(mse.mean(axis=0)[:10]), 'mse_t6': np.mean(mse.mean(axis=0)[:6]),
                'ssim_t10': np.mean(ssim.mean(axis=0)[:10]), 'ssim_t6': np.mean(ssim.mean(axis=0)[:6])}
        for k, v in want.items():
            assert abs(printed[k] - float(v)) <= 1e-6 * abs(float(v)), (k, printed[k], v)
        small = float(np.mean(np.abs(ssim) < 1e-2))
        print('eval: printed', printed)
        print('per-window MSE min', float(mse.min()), 'max', float(mse.max()), 'largest relative MSE difference to fp64',
              float(np.abs(mse / mse64 - 1).max()))
        print('per-pair SSIM from', float(ssim.min()), 'to', float(ssim.max()), 'share below 1e-2 in magnitude', small, 'E', E)
        assert float(mse.min()) >= MSE_FLOOR, 'the smallest per-window MSE is %g' % float(mse.min())
        assert E <= E_CEILING, E
        assert min(abs(printed['ssim_t10']), abs(printed['ssim_t6'])) >= SSIM_FLOOR, printed
        printed['E'] = E
        np.savez_compressed(os.path.join(out, 'metrics.npz'), mse=mse, ssim=ssim, ssim_fp64=ssim64)
        shutil.copy(os.path.join(xp, 'params.json'), os.path.join(out, 'params.json'))
        with open(os.path.join(out, 'printed.json'), 'w') as f:
            json.dump(printed, f, indent=1)
        with open(os.path.join(out, 'flags.json'), 'w') as f:
            json.dump(_flags(os.path.join(REF, SCRIPT)), f, indent=1)
    finally:
        shutil.rmtree(xp, ignore_errors=True)


def main():
    if not getattr(torch.load, '_whole_module', False):
        load = functools.partial(torch.load, weights_only=False)
        load._whole_module = True
        torch.load = load
    I.install_fake_netcdf4()
    sys.path.insert(0, REF)
    from var_sep.data import sst as ref_sst
    from var_sep.test.sst import test as ref_test
    from var_sep.utils.helper import DotDict, save

    os.makedirs(I.GOLDEN, exist_ok=True)
    data_dir = tempfile.mkdtemp(prefix='sst_data_')          # the stand-in reads no file; the directory only has to be named
    try:
        dataset_fixture(ref_sst, ref_test, data_dir, I.GOLDEN)
        eval_fixture(ref_test, DotDict, save, data_dir, os.path.join(I.GOLDEN, 'eval_cli'))
    finally:
        shutil.rmtree(data_dir, ignore_errors=True)
        I.remove_fake_netcdf4()
    for base, _, names in os.walk(I.GOLDEN):
        for n in sorted(names):
            size = os.path.getsize(os.path.join(base, n))
            print(os.path.join(os.path.relpath(base, I.GOLDEN), n), size)
            assert size <= FILE_LIMIT, n


if __name__ == '__main__':
    main()

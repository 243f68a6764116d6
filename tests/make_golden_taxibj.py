"""Generate tests/golden/taxibj/ by running the REFERENCE's TaxiBJ loader (var_sep.data.taxibj.TaxiBJ.make_datasets) and evaluation script
(var_sep.test.taxibj.test -- its own `compute_mse` and `main`, on the CPU) on the synthetic years of tests/taxibj_inputs.py.

TEST INFRASTRUCTURE ONLY; runs only where the reference is available (VARSEP_REFERENCE, default /root/reference):

    python tests/make_golden_taxibj.py

The reference reads its files through h5py, which need not exist where this runs: taxibj_inputs.install_fake_h5py puts a stand-in with
`File`, `__getitem__` and `close` into sys.modules, through which the UNMODIFIED reference loader runs (float64 windows, fp32 items).
`torch.load` reads whole-module pickles, as tests/make_golden_eval_cli.py arranges it.

Written:
  * dataset.npz: for the two calls of taxibj_inputs.CALLS the lengths of both halves, `_min` / `_max` of the fitted normalisation, the
    zlib.crc32 of every item's fp32 bytes (cond then target) of both halves, and the six whole items of taxibj_inputs.WHOLE_ITEMS;
  * eval_cli/: params.json, printed.json, mse.npz ([1344, 4], the reference's per-window per-frame MSE) and flags.json for the
    `vgg32_tiny` network of oracle/golden_configs.py filled with oracle.detdata.det_fill -- NO checkpoint: the test rebuilds the weights
    with the same det_fill.
The smallest reference per-window MSE must be at least MSE_FLOOR, so that the absolute term of the comparison rule of the evaluation CLIs
(|a - b| <= 1e-3 |b| + 1e-5) never decides a case; with salt 13 of the config it is far above (printed below).
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

import taxibj_inputs as I  # noqa: E402
from eval_cli_inputs import write_params  # noqa: E402
from oracle.detdata import det_fill  # noqa: E402
from oracle.golden_configs import CONFIGS  # noqa: E402

SCRIPT = 'var_sep/test/taxibj/test.py'
FILE_LIMIT = 440 * 1000          # the largest fixture committed before these
MSE_FLOOR = 1e-3


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


def _items(ds):
    """fp32 [n, len_closeness, 2, 32, 32]: every item of a reference dataset through its own `__getitem__`."""
    return np.stack([torch.cat(ds[i]).numpy() for i in range(len(ds))]) if len(ds) else np.zeros((0,), dtype=np.float32)


def dataset_fixture(ref_taxibj, data_dir, out):
    z = {}
    for call, kw in I.CALLS.items():
        train, test = ref_taxibj.TaxiBJ.make_datasets(data_dir, **kw)
        assert train.data.dtype == np.float64 and train[0][0].dtype == torch.float32
        assert tuple(train[0][0].shape) == (kw['nt_cond'], 2, 32, 32)
        halves = {'train': _items(train), 'test': _items(test)}
        z['len_%s' % call] = np.array([len(train), len(test)], dtype=np.int64)
        z['min_%s' % call], z['max_%s' % call] = np.float64(train.mmn._min), np.float64(train.mmn._max)
        for half, items in halves.items():
            z['crc_%s_%s' % (call, half)] = I.item_crcs(items)
        for c, half, index in I.WHOLE_ITEMS:
            if c == call:
                z[I.whole_item_key(c, half, index)] = halves[half][index]
        print(call, 'lengths', z['len_%s' % call], 'min', z['min_%s' % call], 'max', z['max_%s' % call],
              'largest test value', float(halves['test'].max()), 'smallest', float(min(h.min() for h in halves.values())))
    assert float(z['min_a']) == 0.0 and z['max_a'] < I.BIG and z['max_b'] == I.BIG
    path = os.path.join(out, 'dataset.npz')
    np.savez_compressed(path, **z)
    return path


def eval_fixture(ref_test, DotDict, save, data_dir, out):
    from oracle.make_golden import _reference_modules, build_reference
    rf, rm, ru, _ = _reference_modules()
    cfg = CONFIGS['vgg32_tiny']
    assert cfg['nt_cond'] == I.PARAMS['nt_cond'] and cfg['offset'] == I.PARAMS['offset']
    net = det_fill(build_reference(cfg, rf, rm, ru), salt=cfg['salt'])
    os.makedirs(out, exist_ok=True)
    xp = tempfile.mkdtemp(prefix='taxibj_xp_')
    try:
        save(xp, net)
        write_params(xp, I.PARAMS)
        # the per-window array: what `main` computes before it prints, through the script's own functions
        from var_sep.utils.helper import load_json
        from var_sep.test.utils import load_model
        xp_config = load_json(os.path.join(xp, 'params.json'))
        xp_config.device, xp_config.data_dir, xp_config.xp_dir, xp_config.nt_pred = torch.device('cpu'), data_dir, xp, 4
        mse = np.concatenate(ref_test.compute_mse(xp_config, ref_test.load_dataset(xp_config), load_model(xp_config, None)), axis=0)
        torch.set_grad_enabled(True)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            ref_test.main(DotDict(data_dir=data_dir, xp_dir=xp, epoch=None, device=None))
        torch.set_grad_enabled(True)
        line = [q for q in buf.getvalue().splitlines() if q.startswith('MSE at t+4:')][-1]
        printed = float(line.split(':', 1)[1])
        assert mse.shape == (I.N_TEST, 4) and abs(printed - float(np.mean(mse.mean(axis=0)[:4]))) <= 1e-6 * printed
        print('eval: printed', printed, 'per-window MSE min', float(mse.min()), 'max', float(mse.max()))
        assert float(mse.min()) >= MSE_FLOOR, 'choose another salt or gain: the smallest per-window MSE is %g' % float(mse.min())
        np.savez_compressed(os.path.join(out, 'mse.npz'), mse=mse)
        shutil.copy(os.path.join(xp, 'params.json'), os.path.join(out, 'params.json'))
        with open(os.path.join(out, 'printed.json'), 'w') as f:
            json.dump({'mse_t4': printed}, f, indent=1)
        with open(os.path.join(out, 'flags.json'), 'w') as f:
            json.dump(_flags(os.path.join(REF, SCRIPT)), f, indent=1)
    finally:
        shutil.rmtree(xp, ignore_errors=True)


def main():
    if not getattr(torch.load, '_whole_module', False):
        load = functools.partial(torch.load, weights_only=False)
        load._whole_module = True
        torch.load = load
    I.install_fake_h5py()
    sys.path.insert(0, REF)
    from var_sep.data import taxibj as ref_taxibj
    from var_sep.test.taxibj import test as ref_test
    from var_sep.utils.helper import DotDict, save

    os.makedirs(I.GOLDEN, exist_ok=True)
    data_dir = tempfile.mkdtemp(prefix='taxibj_data_')          # the stand-in reads no file; the directory only has to be named
    try:
        dataset_fixture(ref_taxibj, data_dir, I.GOLDEN)
        eval_fixture(ref_test, DotDict, save, data_dir, os.path.join(I.GOLDEN, 'eval_cli'))
    finally:
        shutil.rmtree(data_dir, ignore_errors=True)
        I.remove_fake_h5py()
    for base, _, names in os.walk(I.GOLDEN):
        for n in sorted(names):
            size = os.path.getsize(os.path.join(base, n))
            print(os.path.join(os.path.relpath(base, I.GOLDEN), n), size)
            assert size <= FILE_LIMIT, n


if __name__ == '__main__':
    main()

"""Generate tests/golden/eval_cli_chairs/ and tests/golden/eval_cli_chairs_resnet/ by running the REFERENCE's content-swap script
(var_sep.test.chairs.test_disentanglement -- its own `main(args)`, on the CPU) on the tree of tests/chairs_inputs.py.

TEST INFRASTRUCTURE ONLY; runs only where the reference is available (VARSEP_REFERENCE, default /root/reference):

    python tests/make_golden_eval_cli_chairs.py

`tqdm` is stubbed when it is absent and `torch.load` reads whole-module pickles, as tests/make_golden_eval_cli.py arranges it.  One more
shim: the reference's items are `permute(0, 3, 1, 2)` views of HWC arrays, and a current torch collates them into a batch that keeps
that channels-last layout, on which every encoder's `x.view(x.size(0), -1, ...)` (conv.py:90, 347, 547) fails -- the torch the
reference was written for stacked into a contiguous batch.  The script's DataLoader is therefore given a collate function that makes
the default collation contiguous: the same values in the layout the reference expects.

Written:
  * eval_cli_chairs/: a reference-written checkpoint of a small 3-channel DCGAN network (torch.manual_seed fixed, four files, <= 1 MB
    together), params.json, the five output .npz files, printed.json and flags.json (the reference parser's flags, defaults, types and
    required-ness, read from the script's source);
  * eval_cli_chairs_resnet/: the same outputs for the `chairs_resnet` network of oracle/golden_configs.py (ResNet18 encoders + DCGAN
    decoder) filled with oracle.detdata.det_fill -- NO checkpoint (tens of MB): the test rebuilds the weights with the same det_fill.
An output file above PART_LIMIT bytes (the forecasts of untrained networks compress badly: 124 items x 2 frames x 12 KB) is committed as
`<name>.part<k>.npz` files of consecutive items, each below the limit, with the reference's key; chairs_inputs.load_output joins them.
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
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = os.environ.get('VARSEP_REFERENCE', '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import chairs_inputs as I  # noqa: E402
from eval_cli_inputs import parse_results, write_params  # noqa: E402
from oracle.detdata import det_fill  # noqa: E402
from oracle.golden_configs import CONFIGS  # noqa: E402

SCRIPT = 'var_sep/test/chairs/test_disentanglement.py'
OUTPUTS = ['results_swap.npz', 'content_swap_gt.npz', 'content_swap_test.npz', 'cond_swap_test.npz', 'target_swap_test.npz']
CKPT_LIMIT = 1 << 20
PART_LIMIT = 440 * 1000          # the largest fixture committed before these
# the small DCGAN network of the first case; gain 1.0 instead of the training default 0.02 so that the forecasts are not a flat grey
TINY = dict(code_size_s=6, code_size_t=5, hidden=4, res_hidden=8, n_blocks=1, seed=21, gain=1.0)


def _stub_modules():
    try:
        import tqdm  # noqa: F401
    except ImportError:
        tq = types.ModuleType('tqdm')
        tq.tqdm = lambda it, *a, **k: it
        sys.modules['tqdm'] = tq
    if not getattr(torch.load, '_whole_module', False):
        load = functools.partial(torch.load, weights_only=False)
        load._whole_module = True
        torch.load = load


def _contiguous_collate(batch):
    from torch.utils.data import default_collate
    return [t.contiguous() for t in default_collate(batch)]


def _flags(path):
    """[[flag, default, type, required], ...] of the script's `p.add_argument` calls."""
    tree = ast.parse(open(path).read())
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, 'attr', None) == 'add_argument':
            kw = {k.arg: k.value for k in node.keywords}
            default = ast.literal_eval(kw['default']) if 'default' in kw else None
            typ = kw['type'].id if 'type' in kw else None
            req = ast.literal_eval(kw['required']) if 'required' in kw else False
            out.append([ast.literal_eval(node.args[0]), default, typ, req])
    return out


def _run(fn, args):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        fn(args)
    print(buf.getvalue()[-300:])
    return buf.getvalue()


def _copy_output(src, out, name):
    """The reference's file as it is, or cut along the item axis into the fewest equal runs of items whose files all fit PART_LIMIT."""
    for old in os.listdir(out):
        if old == name or old.startswith(name[:-4] + '.part'):
            os.remove(os.path.join(out, old))
    if os.path.getsize(src) <= PART_LIMIT:
        shutil.copy(src, os.path.join(out, name))
        return
    with np.load(src) as z:
        (key,) = z.files
        arr = z[key]
    for n_parts in range(2, len(arr) + 1):
        per = -(-len(arr) // n_parts)
        paths = []
        for k in range(n_parts):
            paths.append(os.path.join(out, '%s.part%d.npz' % (name[:-4], k)))
            np.savez_compressed(paths[-1], **{key: arr[k * per:(k + 1) * per]})
        if all(os.path.getsize(q) <= PART_LIMIT for q in paths):
            return
        for q in paths:
            os.remove(q)
    raise RuntimeError('%s: one item alone exceeds %d bytes' % (name, PART_LIMIT))


def _case(out, sep_net, params, data, ref_dis, DotDict, save, keep_checkpoint):
    os.makedirs(out, exist_ok=True)
    xp = tempfile.mkdtemp(prefix='chairs_xp_')
    try:
        save(xp, sep_net)
        write_params(xp, params)
        args = DotDict(data_dir=data, xp_dir=xp, epoch=None, batch_size=I.RUN['batch_size'], nt_pred=I.RUN['nt_pred'], device=None,
                       test_seed=I.RUN['test_seed'])
        text = _run(ref_dis.main, args)
        for name in OUTPUTS:
            _copy_output(os.path.join(xp, name), out, name)
        for name in ['params.json'] + (['ov_Es.pt', 'ov_Et.pt', 't_resnet.pt', 'decoder.pt'] if keep_checkpoint else []):
            shutil.copy(os.path.join(xp, name), os.path.join(out, name))
        with open(os.path.join(out, 'printed.json'), 'w') as f:
            json.dump(parse_results(text), f, indent=1)
    finally:
        shutil.rmtree(xp, ignore_errors=True)
    sizes = {n: os.path.getsize(os.path.join(out, n)) for n in sorted(os.listdir(out))}
    print(os.path.basename(out), sizes)
    return sizes


def main():
    _stub_modules()
    sys.path.insert(0, REF)
    from var_sep.utils.helper import DotDict, save
    from var_sep.test.chairs import test_disentanglement as ref_dis
    from var_sep.networks.factory import get_encoder, get_decoder, get_resnet
    from var_sep.networks.model import SeparableNetwork

    from torch.utils.data import DataLoader
    ref_dis.DataLoader = functools.partial(DataLoader, collate_fn=_contiguous_collate)

    data = tempfile.mkdtemp(prefix='chairs_data_')
    try:
        I.write_tree(data)
        shape = [3, I.SIZE, I.SIZE]

        # ---- small DCGAN network, reference-written checkpoint ------------------------------------------------------------------------
        out = os.path.join(I.GOLDEN, 'eval_cli_chairs')
        t = TINY
        torch.manual_seed(t['seed'])
        Es = get_encoder('dcgan', shape, t['code_size_s'], t['hidden'], 3, I.RUN['nt_cond'], 'normal', t['gain'])
        Et = get_encoder('dcgan', shape, t['code_size_t'], t['hidden'], 3, I.RUN['nt_cond'], 'normal', t['gain'])
        dec = get_decoder('dcgan', shape, t['code_size_t'], t['code_size_s'], 'sigmoid', t['hidden'], 3, 'concat', False, 'normal', t['gain'])
        res = get_resnet(t['code_size_t'], t['n_blocks'], t['res_hidden'], 'orthogonal', 1.41)
        sizes = _case(out, SeparableNetwork(Es, Et, res, dec, I.RUN['nt_cond'], False), I.PARAMS, data, ref_dis, DotDict, save, True)
        assert sum(v for k, v in sizes.items() if k.endswith('.pt')) <= CKPT_LIMIT, sizes
        with open(os.path.join(out, 'flags.json'), 'w') as f:
            json.dump(_flags(os.path.join(REF, SCRIPT)), f, indent=1)

        # ---- the recipe's encoder: ResNet18 + DCGAN decoder, det_fill weights, no checkpoint committed --------------------------------
        from oracle.make_golden import _reference_modules, build_reference
        rf, rm, ru, _ = _reference_modules()
        cfg = CONFIGS['chairs_resnet']
        assert cfg['nt_cond'] == I.RUN['nt_cond']
        net = det_fill(build_reference(cfg, rf, rm, ru), salt=cfg['salt'])
        _case(os.path.join(I.GOLDEN, 'eval_cli_chairs_resnet'), net, I.PARAMS_RESNET, data, ref_dis, DotDict, save, False)
    finally:
        shutil.rmtree(data, ignore_errors=True)


if __name__ == '__main__':
    main()

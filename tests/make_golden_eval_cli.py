"""Generate tests/golden/eval_cli_* by running the REFERENCE's evaluation scripts (var_sep.test.mnist.test, .test_disentanglement,
var_sep.test.wave.test -- their own `main(args)`, on the CPU) on the inputs of tests/eval_cli_inputs.py.

TEST INFRASTRUCTURE ONLY; runs only where the reference is available (VARSEP_REFERENCE, default /root/reference):

    python tests/make_golden_eval_cli.py

torchvision is not needed: a placeholder `torchvision.datasets.MNIST` serves the digits of the idx files the inputs helper writes (the
reference only reads images through it), as oracle/make_golden_mmnist.py does; `tqdm` is stubbed the same way when it is absent.  The
reference's checkpoints are whole-module pickles, which torch >= 2.6 only loads with weights_only=False.

Written: eval_cli_flags.json (the reference parsers' flags and defaults, read from the scripts' source), eval_cli_mnist/ (params.json,
the seven + five output .npz files, printed results), eval_cli_wave/ and eval_cli_wave_partial/ (reference-written MLP checkpoints,
params.json, per-window MSE arrays, printed result).
"""
import ast
import contextlib
import functools
import io
import json
import os
import shutil
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = os.environ.get('VARSEP_REFERENCE', '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import eval_cli_inputs as I  # noqa: E402
from oracle.wave_data_ref import fixture_dir, sorted_listdir  # noqa: E402

SCRIPTS = {'mnist_test': 'var_sep/test/mnist/test.py', 'mnist_test_disentanglement': 'var_sep/test/mnist/test_disentanglement.py',
           'wave_test': 'var_sep/test/wave/test.py'}


def _stub_modules():
    if 'torchvision' not in sys.modules:
        tv = types.ModuleType('torchvision')
        tv.datasets = types.ModuleType('torchvision.datasets')

        class MNIST:
            def __init__(self, root, train=True, download=False):
                name = 'train-images-idx3-ubyte' if train else 't10k-images-idx3-ubyte'
                self.images = I.read_idx(os.path.join(root, 'MNIST', 'raw', name))

            def __len__(self):
                return len(self.images)

            def __getitem__(self, i):
                if i >= len(self.images):
                    raise IndexError(i)
                return self.images[i], 0

        tv.datasets.MNIST = MNIST
        sys.modules['torchvision'], sys.modules['torchvision.datasets'] = tv, tv.datasets
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
        ret = fn(args)
    print(buf.getvalue()[-600:])
    return buf.getvalue(), ret


def main():
    _stub_modules()
    sys.path.insert(0, REF)
    from var_sep.utils.helper import DotDict, save
    from var_sep.test.mnist import test as ref_test
    from var_sep.test.mnist import test_disentanglement as ref_dis
    from var_sep.test.wave import test as ref_wave
    from var_sep.networks.factory import get_encoder, get_decoder, get_resnet
    from var_sep.networks.model import SeparableNetwork

    flags = {k: _flags(os.path.join(REF, v)) for k, v in SCRIPTS.items()}
    with open(os.path.join(I.GOLDEN, 'eval_cli_flags.json'), 'w') as f:
        json.dump(flags, f, indent=1)

    tmp = fixture_dir() + '_evalcli'          # digit-free: the WaveEq split reads the first integer of the path
    shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(tmp)
    try:
        # ---- Moving MNIST ------------------------------------------------------------------------------------------------------------
        data = I.write_mnist_inputs(os.path.join(tmp, 'mnist'))
        out = os.path.join(I.GOLDEN, 'eval_cli_mnist')
        os.makedirs(out, exist_ok=True)
        I.write_params(out, I.MNIST_PARAMS)
        printed = {}
        for tag, mod in (('test', ref_test), ('test_disentanglement', ref_dis)):
            xp = os.path.join(tmp, 'xp_' + tag)
            shutil.copytree(os.path.join(I.GOLDEN, 'ckpt_dcgan_tiny'), xp)
            I.write_params(xp, I.MNIST_PARAMS)
            args = DotDict(data_dir=data, xp_dir=xp, epoch=None, batch_size=I.MNIST_RUN['batch_size'][tag], nt_pred=I.MNIST_RUN['nt_pred'],
                           device=None, test_seed=I.MNIST_RUN['test_seed'])
            text, _ = _run(mod.main, args)
            printed[tag] = I.parse_results(text)
            for name in os.listdir(xp):
                if name.endswith('.npz'):
                    shutil.copy(os.path.join(xp, name), os.path.join(out, name))
        with open(os.path.join(out, 'printed.json'), 'w') as f:
            json.dump(printed, f, indent=1)

        # ---- WaveEq ------------------------------------------------------------------------------------------------------------------
        wdata = I.write_wave_inputs(os.path.join(tmp, 'wave'))
        for kind, params in I.WAVE_PARAMS.items():
            out = os.path.join(I.GOLDEN, 'eval_cli_' + kind)
            os.makedirs(out, exist_ok=True)
            shape = [1, I.WAVE['H'], I.WAVE['W']] if kind == 'wave' else [1, params['n_wave_points']]
            torch.manual_seed(11 if kind == 'wave' else 12)
            Es = get_encoder('mlp', shape, 8, 32, 3, params['nt_cond'], 'normal', 0.2)
            Et = get_encoder('mlp', shape, 6, 32, 3, params['nt_cond'], 'normal', 0.2)
            dec = get_decoder('mlp', shape, 6, 8, 'sigmoid', 32, 3, 'concat', False, 'normal', 0.2)
            res = get_resnet(6, 2, 16, 'orthogonal', 1.41)
            sep_net = SeparableNetwork(Es, Et, res, dec, params['nt_cond'], False)
            save(out, sep_net)
            I.write_params(out, params)
            args = DotDict(data_dir=wdata, xp_dir=out, epoch=None, batch_size=I.WAVE_RUN['batch_size'], device=None)
            text, _ = _run(ref_wave.main, args)
            # the per-window arrays, through the reference's own functions as its main() calls them, under a sorted file listing
            # (the window order follows os.listdir; the printed mean does not depend on it)
            xp_config = ref_wave.load_json(os.path.join(out, 'params.json'))
            xp_config.device, xp_config.data_dir, xp_config.xp_dir, xp_config.nt_pred = torch.device('cpu'), wdata, out, 40
            with sorted_listdir():
                test_set = ref_wave.load_dataset(xp_config, train=False)
            net = ref_wave.load_model(xp_config, None)
            mse = np.concatenate(ref_wave.compute_mse(xp_config, I.WAVE_RUN['batch_size'], test_set, net), axis=0)
            np.savez_compressed(os.path.join(out, 'mse.npz'), mse=mse)
            with open(os.path.join(out, 'printed.json'), 'w') as f:
                json.dump(I.parse_results(text), f, indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for d in ('eval_cli_mnist', 'eval_cli_wave', 'eval_cli_wave_partial'):
        p = os.path.join(I.GOLDEN, d)
        print(d, {n: os.path.getsize(os.path.join(p, n)) for n in sorted(os.listdir(p))})


if __name__ == '__main__':
    main()

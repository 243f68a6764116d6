"""What the GPU tests of the evaluation CLIs and of `main` share: where the package is, the project's closeness rule, a module run in a
fresh process, a checkpoint directory of det_fill weights, the checks of a training run."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'spatiotemporal_variable_separation_amd'


def close(a, b, rel=1e-3, floor=1e-5):
    """|a - b| <= rel |b| + floor, element-wise, on equal shapes.  rel 1e-3 is the rule of the evaluation CLIs; `floor` absorbs values
    near zero (the mean SSIM of an untrained model is ~1e-3, a sum of terms of both signs)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= rel * np.abs(b) + floor))


def run_module(module, args, timeout=600):
    """stdout of `python -m <PKG>.<module> args` run from the repository root; a non-zero exit fails the test with the output's end."""
    r = subprocess.run([sys.executable, '-m', '%s.%s' % (PKG, module)] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def write_xp(config, path, params_json):
    """`path`: the network `config` of oracle/golden_configs.py with its det_fill weights, saved by this package's own `save`, and a copy
    of `params_json` beside it."""
    from oracle.detdata import det_fill
    from oracle.golden_configs import CONFIGS
    from spatiotemporal_variable_separation_amd.networks.factory import build_sep_net
    from spatiotemporal_variable_separation_amd.utils.helper import save
    cfg = CONFIGS[config]
    save(path, det_fill(build_sep_net(cfg), salt=cfg['salt']))
    shutil.copy(params_json, path)
    return path


def check_training_run(stdout, xp_dir, min_losses):
    """Output and files of one epoch of `main` with --chkpt_interval 1: the recorded-graph default, finite losses, the checkpoint files."""
    assert 'recorded hipGraph' in stdout and 'frames/s' in stdout, stdout[-2000:]
    losses = [float(v) for v in re.findall(r'total (\S+)', stdout)]
    assert len(losses) >= min_losses and all(np.isfinite(v) for v in losses), stdout[-2000:]
    for stem in ('ov_Et', 'ov_Es', 'decoder', 't_resnet'):
        assert (xp_dir / f'{stem}.pt').exists() and (xp_dir / f'{stem}_1.pt').exists()
    assert (xp_dir / 'params.json').exists()

"""Helpers shared by the evaluation scripts (reference: test/utils.py:8-24)."""
import argparse

import numpy as np
import torch

from .. import functional as VF
from .. import ops
from ..utils.helper import load_sep_net
from ..utils.metrics import _ssim_wrapper  # noqa: F401  (test/utils.py:19-24, on the device)

NO_CPU_MODE = 'the MI355X-native path has no CPU mode: pass --device N'


def load_model(xp_config, epoch_number=None):
    """test/utils.py:8-16: the four checkpoint files of `xp_config.xp_dir` (this package's or the reference's) as a SeparableNetwork on
    `xp_config.device`, in eval mode."""
    sep_net = load_sep_net(xp_config.xp_dir, xp_config.nt_cond, xp_config.skipco, epoch_number)
    sep_net = sep_net.to(xp_config.device)
    sep_net.eval()
    return sep_net


def setup_device(args):
    """The reference evaluates on the CPU when --device is absent; this path has no CPU fallback (main.py).  Returns cuda:<device>
    and selects the compute precision."""
    if args.device is None:
        raise RuntimeError(NO_CPU_MODE)
    from .. import configure_single_gpu_queues
    configure_single_gpu_queues()      # before the first HIP call of the process, as main.py does
    device = torch.device('cuda', args.device)
    torch.cuda.set_device(device)
    VF.set_precision(args.precision or 'fp32')
    return device


def add_precision_flag(p):
    """Additive flag (not in the reference): fp32 is the reference's arithmetic, bf16 selects the 16-bit kernels."""
    p.add_argument('--precision', type=str, choices=['fp32', 'bf16'], default='fp32',
                   help='Compute precision of the forward pass (fp32: the reference\'s arithmetic; bf16: 16-bit MFMA kernels).')


def base_parser(prog, batch_size, nt_pred=True):
    """--data_dir --xp_dir --epoch --batch_size [--nt_pred] --device (+ --precision) with the reference's defaults."""
    p = argparse.ArgumentParser(prog=prog)
    p.add_argument('--data_dir', type=str, metavar='DIR', required=True,
                   help='Directory where the dataset is saved.')
    p.add_argument('--xp_dir', type=str, metavar='DIR', required=True,
                   help='Directory where the model configuration file and checkpoints are saved.')
    p.add_argument('--epoch', type=int, metavar='EPOCH', default=None,
                   help='If specified, loads the checkpoint of the corresponding epoch number.')
    p.add_argument('--batch_size', type=int, metavar='BATCH', default=batch_size,
                   help='Batch size used to compute metrics.')
    if nt_pred:
        p.add_argument('--nt_pred', type=int, metavar='PRED', required=True,
                       help='Total of frames to predict.')
    p.add_argument('--device', type=int, metavar='DEVICE', default=None,
                   help='GPU where the model should be placed when testing (required: there is no CPU mode)')
    return p


def to_host_u8(x):
    """`x.cpu().mul(255).byte().permute(0, 1, 3, 4, 2)` of a [B, T, C, H, W] device tensor: converted on the device
    (ops.frames_to_u8_nhwc), only the uint8 bytes are copied."""
    return ops.frames_to_u8_nhwc(x).cpu()


def print_results(results):
    """The reference's closing block (test/mnist/test.py:151-159): concatenated per-sample arrays and their means."""
    print('\n')
    print('Results:')
    out = {}
    for name, parts in results.items():
        res = torch.cat(parts).numpy()
        out[name] = res
        print(name, res.mean())
    return out


def seed_all(seed):
    """random, NumPy and torch seeded in the reference's order (test/mnist/test.py:61-64)."""
    import random
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)

"""Helpers shared by the evaluation scripts (reference: test/utils.py:8-24)."""
import argparse
import os

import numpy as np
import torch

from .. import functional as VF
from .. import ops
from ..data.device import DeviceBatchLoader
from ..utils import savez
from ..utils.helper import load_json, load_sep_net
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


def load_xp_config(args, device, nt_pred):
    """The `params.json` of `args.xp_dir` with the run's own device, directories and horizon (test/mnist/test.py:66-70)."""
    xp_config = load_json(os.path.join(args.xp_dir, 'params.json'))
    xp_config.device = device
    xp_config.data_dir = args.data_dir
    xp_config.xp_dir = args.xp_dir
    xp_config.nt_pred = nt_pred
    return xp_config


def add_precision_flag(p):
    """Additive flag (not in the reference): fp32 is the reference's arithmetic, bf16 selects the 16-bit kernels.  Returns `p`."""
    p.add_argument('--precision', type=str, choices=['fp32', 'bf16'], default='fp32',
                   help='Compute precision of the forward pass (fp32: the reference\'s arithmetic; bf16: 16-bit MFMA kernels).')
    return p


def base_parser(prog, batch_size, nt_pred=True, test_seed=False):
    """--data_dir --xp_dir --epoch --batch_size [--nt_pred] --device [--test_seed] with the reference's defaults."""
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
    if test_seed:
        p.add_argument('--test_seed', type=int, metavar='SEED', default=1,
                       help='Manual seed.')
    return p


def to_host_u8(x):
    """`x.cpu().mul(255).byte().permute(0, 1, 3, 4, 2)` of a [B, T, C, H, W] device tensor: converted on the device
    (ops.frames_to_u8_nhwc), only the uint8 bytes are copied."""
    return ops.frames_to_u8_nhwc(x).cpu()


class U8Frames:
    """The uint8 frames an evaluation script saves, collected batch by batch.  compress='host': every batch is converted on the device and
    copied to the host at once (`to_host_u8`), `cat()` is the NumPy array of `torch.cat` -- the calls of the time before the device
    encoder, in their order.  compress='device': the uint8 batches stay in HBM and `cat()` is a device tensor for
    utils/savez.savez_compressed; nothing is copied to the host per batch.  n_items: the number of samples when the caller knows it;
    the device route then converts every batch straight into one preallocated [n_items, T, H, W, C] buffer (allocated at the first
    batch, whose frame shape it takes) and `cat()` is that buffer, with no `torch.cat` copy beside it."""

    def __init__(self, compress, n_items=None):
        if compress not in ('host', 'device'):
            raise ValueError("compress=%r: 'host' or 'device' expected" % (compress,))
        self.compress, self.n_items = compress, n_items
        self.parts, self.buffer, self.filled = [], None, 0

    def append(self, x):
        """x: [B, T, C, H, W] on the device."""
        if self.compress == 'host':
            self.parts.append(to_host_u8(x))
        elif self.n_items is None:
            self.parts.append(ops.frames_to_u8_nhwc(x))
        else:
            B, T, C, H, W = x.shape
            if self.buffer is None:
                self.buffer = torch.empty((int(self.n_items), T, H, W, C), dtype=torch.uint8, device=x.device)
            if self.filled + B > self.buffer.shape[0]:
                raise ValueError('U8Frames: %d samples appended to a collector made for %d' % (self.filled + B, self.buffer.shape[0]))
            ops.frames_to_u8_nhwc(x, out=self.buffer[self.filled:self.filled + B])
            self.filled += B

    def cat(self):
        """All frames in the order of the appends: a NumPy array (host) or a device tensor (device)."""
        if self.compress == 'host':
            return torch.cat(self.parts).numpy()
        if self.n_items is None:
            if len(self.parts) != 1:
                self.parts = [torch.cat(self.parts)]          # (the batches are released: one copy of the frames stays in HBM)
            return self.parts[0]
        if self.buffer is None:
            raise RuntimeError('U8Frames: nothing was appended')
        return self.buffer[:self.filled]


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


def forecast_targets(sep_net, cond, n_target, cfg):
    """Forecast of the `n_target` frames after `cond`.  With `cfg.offset` the model forecasts from the first conditioning frame on, and
    the conditioning frames are cut off (test/wave/test.py:43-47)."""
    if cfg.offset:
        forecasts = sep_net.get_forecast(cond, n_target + cfg.nt_cond)[0]
        return forecasts[:, cfg.nt_cond:]
    return sep_net.get_forecast(cond, n_target)[0]


def forecast_metrics(cfg, batch_size, test_set, sep_net, metrics):
    """One list per value of `metrics(forecasts, target, *rest)`, holding that value of every sequential batch (cond, target, *rest) of
    the HBM-resident `test_set` as a NumPy array; `forecasts` is fp32 in the shape of `target`."""
    out = None
    loader = DeviceBatchLoader(test_set, batch_size, shuffle=False)
    torch.set_grad_enabled(False)
    for cond, target, *rest in loader:
        forecasts = forecast_targets(sep_net, cond, target.size(1), cfg).float().reshape(target.shape)
        values = metrics(forecasts, target, *rest)
        out = out or [[] for _ in values]
        for parts, value in zip(out, values):
            parts.append(value.cpu().numpy())
    return out


def horizon_mse_main(args, horizon, load_dataset, compute_mse):
    """`main` of the scripts that print the mean MSE of the test windows at a fixed horizon (test/wave/test.py:61-90); returns [N, T(, 1)]."""
    device = setup_device(args)
    xp_config = load_xp_config(args, device, horizon)     # the reference evaluates at this horizon whatever the training horizon
    args.nt_pred = horizon

    test_set = load_dataset(xp_config)
    sep_net = load_model(xp_config, args.epoch)

    all_mse = compute_mse(xp_config, args.batch_size, test_set, sep_net)
    mse_array = np.concatenate(all_mse, axis=0)
    print(f'MSE at t+{horizon}: {np.mean(mse_array.mean(axis=0)[:horizon])}')
    return mse_array


def best_of_permutations(pred, gt_swap):
    """Per sample: min over the permutations of the MSE, max of the PSNR and of the SSIM (test_disentanglement.py:153-166).
    pred [B, T, C, H, W], gt_swap [B, P, T, C, H, W]."""
    mse, ssim = ops.frame_metrics_multi(pred, gt_swap, max_val=1.0)       # [B, P, T, C]
    m = mse.mean(3).mean(2)
    psnr = (10 * torch.log10(1 / mse)).mean(3).mean(2)
    s = ssim.mean(3).mean(2)
    return {'mse': m.min(1)[0], 'psnr': psnr.max(1)[0], 'ssim': s.max(1)[0]}


def run_content_swap(xp_dir, sep_net, nt_cond, nt_test, batches, compress=None):
    """The loop and the five files both content-swap scripts share (test/mnist/test_disentanglement.py:118-223).  `batches` yields
    (x_cond, x_gt_swap, x_swap_cond, x_swap_target): S is extracted from `x_cond`, drives a forecast from `x_swap_cond`, and the forecast
    is scored against every candidate of `x_gt_swap` [B, P, ...], best per sample.  Reference quirks kept: `cond_swap_test` holds the S
    video's conditioning frames `x_cond`, not `x_swap_cond`; `gt_swap` is the first candidate.
    compress: who compresses the files (utils/savez.npz_compressor).  The content-swap scripts' `main`s hand nothing on, so the rule
    (VARSEP_NPZ_COMPRESS) is read here, once, before the first batch is drawn: a bad value is refused before any forecast.  The number
    of samples is not known here (`batches` is a generator), so on the device route the batches are kept and concatenated at the end."""
    compress = savez.npz_compressor(compress)
    gt_swap, content_swap, cond_swap, target_swap = (U8Frames(compress) for _ in range(4))
    results = {'mse': [], 'psnr': [], 'ssim': []}
    for x_cond, x_gt_swap, x_swap_cond, x_swap_target in batches:
        # Extraction of S
        _, _, s_code, _ = sep_net.get_forecast(x_cond, nt_test)

        # Content swap
        cond_swap.append(x_cond)
        target_swap.append(x_swap_target)
        x_swap_pred = sep_net.get_forecast(x_swap_cond, nt_test, init_s_code=s_code)[0]
        x_swap_pred = x_swap_pred[:, nt_cond:].float().contiguous()
        content_swap.append(x_swap_pred)
        gt_swap.append(x_gt_swap[:, 0])

        # Pixelwise quantitative eval: every candidate scored, best per sample
        metrics_batch = best_of_permutations(x_swap_pred, x_gt_swap.float())
        for name in results:
            results[name].append(metrics_batch[name].cpu())

    results = print_results(results)

    savez.savez_compressed(os.path.join(xp_dir, 'results_swap.npz'), results, compress)
    savez.savez_compressed(os.path.join(xp_dir, 'content_swap_gt.npz'), {'gt_swap': gt_swap.cat()}, compress)
    savez.savez_compressed(os.path.join(xp_dir, 'content_swap_test.npz'), {'content_swap': content_swap.cat()}, compress)
    savez.savez_compressed(os.path.join(xp_dir, 'cond_swap_test.npz'), {'cond_swap': cond_swap.cat()}, compress)
    savez.savez_compressed(os.path.join(xp_dir, 'target_swap_test.npz'), {'target_swap': target_swap.cat()}, compress)
    return results

"""Moving-MNIST content-swap (disentanglement) evaluation (reference: test/mnist/test_disentanglement.py:53-223, same flags and files):

    python -m spatiotemporal_variable_separation_amd.test.mnist.test_disentanglement --xp_dir X --data_dir D --nt_pred 95 --device 0

S is extracted from a video whose digits follow a test trajectory backwards; T comes from a test video; the forecast is scored against
every assignment of the S video's digits to the test video's trajectories, and the best score per sample is kept.

Two limits of the reference are lifted, and the results are the reference's wherever it runs:
  * with a ragged last test batch the reference fails (the S code of a full swap batch meets a shorter test batch); here the swap batch
    is trimmed to the test batch;
  * with n_object >= 3 the reference fails at `view(-1, n_object, ...)` because it renders n! permutations; here all n! are scored.
"""
import itertools
import math
import os

import numpy as np
import torch

from ... import ops
from ...data.moving_mnist import read_mnist_images
from ...utils.helper import load_json
from ..utils import add_precision_flag, base_parser, load_model, print_results, seed_all, setup_device, to_host_u8
from .test import load_dataset, test_batches


class SwapDataset:
    """test_disentanglement.py:53-90 with the videos rendered on the device.  Item `index` is the reversed-trajectory video (trajectory
    `len - index - 1`) and the n! videos of every digit permutation along trajectory `index`, with the digits
    `digits_permutation[index + i * len]` of the MNIST test images; `batch(indices)` renders a whole batch in one launch
    (ops.moving_mnist_place)."""

    frame_size = 64
    object_size = 28

    def __init__(self, data_dir, seq_len, nt_cond, n_object, device='cuda', out_dtype=torch.float32):
        self.seq_len, self.n_object, self.nt_cond, self.out_dtype = seq_len, n_object, nt_cond, out_dtype
        self.digits_permutation = np.random.permutation(10000)
        latents = np.load(os.path.join(data_dir, f'mmnist_test_{n_object}digits_{self.frame_size}.npz'), allow_pickle=True)['latents']
        if latents.shape[0] < seq_len or latents.shape[2] != n_object:
            raise ValueError('latents %s: need >= %d frames of %d objects' % (latents.shape, seq_len, n_object))
        # (sx, sy) of the frames and trajectories an item can read, uploaded once
        pos = np.ascontiguousarray(latents[:seq_len, :len(self), :, :2], dtype=np.int32)
        self.positions = torch.from_numpy(pos).to(device)
        self.images = torch.from_numpy(read_mnist_images(data_dir, train=False)).to(device)
        self.reorderings = list(itertools.permutations(range(n_object)))
        self.device = torch.device(device)

    def __len__(self):
        return 10000 // self.n_object

    def descriptors(self, indices):
        """int32 [len(indices) * (1 + n!), 1 + n_object]: (trajectory, digit of object 0 .. n-1) of every video of the items."""
        n, L = self.n_object, len(self)
        rows = []
        for index in indices:
            img = [int(self.digits_permutation[index + i * L]) for i in range(n)]
            rows.append([L - index - 1] + img)
            for reordering in self.reorderings:
                rows.append([index] + [img[reordering[i]] for i in range(n)])
        return np.asarray(rows, dtype=np.int32)

    def batch(self, indices):
        """(cond, target, swap_cond, swap_target) of the items, as the reference's DataLoader collates them:
        [B, nt_cond, 1, 64, 64], [B, seq_len - nt_cond, ...], [B, n!, nt_cond, ...], [B, n!, seq_len - nt_cond, ...]."""
        desc = torch.from_numpy(self.descriptors(indices)).to(self.device)
        v = ops.moving_mnist_place(self.images, self.positions, desc, self.seq_len, self.frame_size, self.out_dtype)
        v = v.view(len(indices), 1 + len(self.reorderings), self.seq_len, 1, self.frame_size, self.frame_size)
        return v[:, 0, :self.nt_cond], v[:, 0, self.nt_cond:], v[:, 1:, :self.nt_cond], v[:, 1:, self.nt_cond:]


def best_of_permutations(pred, gt_swap):
    """Per sample: min over the permutations of the MSE, max of the PSNR and of the SSIM (test_disentanglement.py:153-166).
    pred [B, T, C, H, W], gt_swap [B, P, T, C, H, W]."""
    mse, ssim = ops.frame_metrics_multi(pred, gt_swap, max_val=1.0)       # [B, P, T, C]
    m = mse.mean(3).mean(2)
    psnr = (10 * torch.log10(1 / mse)).mean(3).mean(2)
    s = ssim.mean(3).mean(2)
    return {'mse': m.min(1)[0], 'psnr': psnr.max(1)[0], 'ssim': s.max(1)[0]}


def main(args):
    device = setup_device(args)
    seed_all(args.test_seed)
    xp_config = load_json(os.path.join(args.xp_dir, 'params.json'))
    xp_config.device = device
    xp_config.data_dir = args.data_dir
    xp_config.xp_dir = args.xp_dir
    xp_config.nt_pred = args.nt_pred

    print('Loading data...')
    test_dataset = load_dataset(xp_config, train=False, device=device)
    swap_dataset = SwapDataset(args.data_dir, xp_config.nt_cond + args.nt_pred, xp_config.nt_cond, xp_config.n_object, device=device)

    print('Loading model...')
    sep_net = load_model(xp_config, args.epoch)

    print('Generating samples...')
    torch.set_grad_enabled(False)
    nt_test = xp_config.nt_cond + args.nt_pred
    gt_swap, content_swap, cond_swap, target_swap = [], [], [], []
    results = {'mse': [], 'psnr': [], 'ssim': []}
    swap_start = 0
    for batch in test_batches(test_dataset, args.batch_size):
        # the swap loader is sequential with the same batch size: batch k holds items [k * batch_size, (k + 1) * batch_size)
        x_swap_cond, x_swap_target = batch
        bsz = len(x_swap_cond)
        if swap_start + bsz > len(swap_dataset):
            raise StopIteration('the swap set (%d items) is exhausted' % len(swap_dataset))
        # trimmed to the test batch (the reference fails on a ragged last batch, see the module docstring)
        x_cond, x_target, _, x_gt_swap = swap_dataset.batch(range(swap_start, swap_start + bsz))
        swap_start += args.batch_size

        # Extraction of S
        _, _, s_code, _ = sep_net.get_forecast(x_cond, nt_test)

        # Content swap (reference quirk kept: `cond_swap_test` holds the S video's conditioning frames)
        cond_swap.append(to_host_u8(x_cond))
        target_swap.append(to_host_u8(x_swap_target))
        x_swap_pred = sep_net.get_forecast(x_swap_cond, nt_test, init_s_code=s_code)[0]
        x_swap_pred = x_swap_pred[:, xp_config.nt_cond:].float().contiguous()
        content_swap.append(to_host_u8(x_swap_pred))
        gt_swap.append(to_host_u8(x_gt_swap[:, 0]))

        # Pixelwise quantitative eval: every permutation scored, best per sample
        metrics_batch = best_of_permutations(x_swap_pred, x_gt_swap.float())
        for name in results:
            results[name].append(metrics_batch[name].cpu())

    results = print_results(results)

    np.savez_compressed(os.path.join(args.xp_dir, 'results_swap.npz'), **results)
    np.savez_compressed(os.path.join(args.xp_dir, 'content_swap_gt.npz'), gt_swap=torch.cat(gt_swap).numpy())
    np.savez_compressed(os.path.join(args.xp_dir, 'content_swap_test.npz'), content_swap=torch.cat(content_swap).numpy())
    np.savez_compressed(os.path.join(args.xp_dir, 'cond_swap_test.npz'), cond_swap=torch.cat(cond_swap).numpy())
    np.savez_compressed(os.path.join(args.xp_dir, 'target_swap_test.npz'), target_swap=torch.cat(target_swap).numpy())
    return results


def build_parser():
    p = base_parser('PDE-Driven Spatiotemporal Disentanglement (Moving MNIST content swap testing)', batch_size=16)
    p.add_argument('--test_seed', type=int, metavar='SEED', default=1,
                   help='Manual seed.')
    add_precision_flag(p)
    return p


if __name__ == '__main__':
    main(build_parser().parse_args())

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
import os

import numpy as np
import torch

from ... import ops
from ...data.moving_mnist import read_mnist_images
from ..utils import add_precision_flag, base_parser, load_model, load_xp_config, run_content_swap, seed_all, setup_device
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


def swap_batches(test_dataset, swap_dataset, batch_size):
    """(x_cond, x_gt_swap, x_swap_cond, x_swap_target) per test batch.  The swap loader is sequential with the same batch size: batch k
    holds items [k * batch_size, (k + 1) * batch_size), trimmed to the test batch (the reference fails on a ragged last batch, see the
    module docstring)."""
    swap_start = 0
    for x_swap_cond, x_swap_target in test_batches(test_dataset, batch_size):
        bsz = len(x_swap_cond)
        x_cond, _, _, x_gt_swap = swap_dataset.batch(range(swap_start, swap_start + bsz))
        swap_start += batch_size
        yield x_cond, x_gt_swap, x_swap_cond, x_swap_target


def main(args):
    device = setup_device(args)
    seed_all(args.test_seed)
    xp_config = load_xp_config(args, device, args.nt_pred)

    print('Loading data...')
    test_dataset = load_dataset(xp_config, train=False, device=device)
    swap_dataset = SwapDataset(args.data_dir, xp_config.nt_cond + args.nt_pred, xp_config.nt_cond, xp_config.n_object, device=device)

    print('Loading model...')
    sep_net = load_model(xp_config, args.epoch)

    print('Generating samples...')
    torch.set_grad_enabled(False)
    if test_dataset.data.shape[0] > len(swap_dataset):
        raise StopIteration('the swap set (%d items) is exhausted' % len(swap_dataset))
    return run_content_swap(args.xp_dir, sep_net, xp_config.nt_cond, xp_config.nt_cond + args.nt_pred,
                            swap_batches(test_dataset, swap_dataset, args.batch_size))


def build_parser():
    p = base_parser('PDE-Driven Spatiotemporal Disentanglement (Moving MNIST content swap testing)', batch_size=16, test_seed=True)
    return add_precision_flag(p)


if __name__ == '__main__':
    main(build_parser().parse_args())

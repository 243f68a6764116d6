"""The Moving-MNIST content-swap evaluation of test_disentanglement.py on a test set GENERATED in HBM, with no `mmnist_test_*.npz`:

    python -m spatiotemporal_variable_separation_amd.test.mnist.test_disentanglement_generated --xp_dir X --data_dir generated:D \
        --nt_pred 95 --device 0

Same flags, seeds, batches, metrics and output files as test_disentanglement.py.  `--data_dir generated:D` means what it means to test.py:
D holds only the raw MNIST idx files, and the test set that preprocessing/mnist/make_test_set.py would write with its defaults is rendered
by one launch (`MovingMNIST.generated`, vs_moving_mnist_testset), which the test videos and the positions of the swap set share.  A
--data_dir without the prefix is refused: the file is test_disentanglement.py's business.  On a directory where make_test_set.py has also
written the file, both scripts hold the same bytes and write the same results.  It is a module of its own because
test_disentanglement.py is kept exactly as it is (as test/chairs/test_disentanglement_raw.py stands beside its script); that script reads
the file and does not know the prefix.
"""
import itertools

import numpy as np
import torch

from ...data.moving_mnist import MovingMNIST
from . import test_disentanglement as filed
from .test import GENERATED, split_data_dir


class GeneratedSwapDataset(filed.SwapDataset):
    """`SwapDataset` whose positions are the latents of the generated test set and whose images are its test images (both already on
    the device, shared and read-only): the same draw from the global NumPy stream, the same items.  Only the constructor differs, and
    the parent's reads the file, so it is not called."""

    def __init__(self, data_dir, seq_len, nt_cond, n_object, device='cuda', out_dtype=torch.float32):
        self.seq_len, self.n_object, self.nt_cond, self.out_dtype = seq_len, n_object, nt_cond, out_dtype
        self.digits_permutation = np.random.permutation(10000)
        test_set = MovingMNIST.generated(generated_dir(data_dir), self.frame_size, nt_cond, seq_len, 4, n_object, device)
        latents = test_set.latents
        if latents.shape[0] < seq_len or latents.shape[2] != n_object:
            raise ValueError('latents %s: need >= %d frames of %d objects' % (tuple(latents.shape), seq_len, n_object))
        self.positions = latents[:seq_len, :len(self), :, :2].contiguous()
        self.images = test_set.test_images
        self.reorderings = list(itertools.permutations(range(n_object)))
        self.device = torch.device(device)


def generated_dir(data_dir):
    """D of `generated:D`; anything else is refused."""
    directory, generated = split_data_dir(data_dir)
    if not generated:
        raise ValueError('--data_dir must be %sD (D: the raw MNIST idx files); test_disentanglement.py evaluates on the file under a '
                         'plain directory (got %r)' % (GENERATED, data_dir))
    return directory


def main(args):
    """test_disentanglement.py's own `main`, run with its swap set exchanged for the generated one (its `load_dataset` is test.py's, which
    knows the prefix): one body, so the two scripts cannot drift apart."""
    generated_dir(args.data_dir)
    original = filed.SwapDataset
    filed.SwapDataset = GeneratedSwapDataset
    try:
        return filed.main(args)
    finally:
        filed.SwapDataset = original


build_parser = filed.build_parser


if __name__ == '__main__':
    main(build_parser().parse_args())

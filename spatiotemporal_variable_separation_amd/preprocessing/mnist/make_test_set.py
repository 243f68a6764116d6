"""Moving-MNIST test set generated on the device (reference: preprocessing/mnist/make_test_set.py, same flags plus --device):

    python -m spatiotemporal_variable_separation_amd.preprocessing.mnist.make_test_set --data_dir D --device 0

Writes D/mmnist_test_{digits}digits_{frame_size}.npz with the reference's keys, shapes and dtypes -- `sequences` uint8 [T, N, 1, F, F],
`latents` int64 [T, N, digits, 4], `labels` uint8 [N, digits], `digits` uint8 [N, digits, h, w] -- the file `MovingMNIST.make_dataset(
train=False)` and both scripts under test/mnist read.  The reference draws a permutation of the 10 000 MNIST test images and four integers
per digit from the seeded global NumPy stream, then walks every trajectory and composites every frame in Python; here the host makes the
same draws in the same order (`draw_test_set`) and ONE launch (ops.moving_mnist_testset, csrc/vs_data.hip) computes all trajectories and
writes all frames and latents, bit for bit the reference's.  The digits come from the raw t10k idx files (images and labels) under D or
D/MNIST/raw, the files torchvision keeps; nothing is downloaded.  Writing the file dominates the run: measured on one MI355X box
(tools/mmnist_testset_bench.py, profiles/mmnist_testset_timing.md) the launch for 5 000 videos of 100 frames takes 0.7 ms and the download
0.2 s, while np.savez_compressed (zlib over 2 GB on one host thread) takes 13.2 s of 13.4 s.  There is no CPU mode: --device is required.
`--data_dir generated:D` of test/mnist/test.py and the script test/mnist/test_disentanglement_generated.py build the same set straight
in HBM, without the file (`MovingMNIST.generated`).
"""
import argparse
import os
import time

import numpy as np
import torch

from ... import ops
from ...data.device import require_gpu
from ...data.moving_mnist import draw_test_set, read_mnist_images, read_mnist_labels


def read_test_digits(data_dir):
    """(images uint8 [N, h, w], labels uint8 [N]) of the raw MNIST test files; a missing file raises naming both."""
    try:
        images, labels = read_mnist_images(data_dir, train=False), read_mnist_labels(data_dir, train=False)
    except FileNotFoundError as e:
        raise FileNotFoundError('%s -- the test set is made from t10k-images-idx3-ubyte[.gz] and t10k-labels-idx1-ubyte[.gz] under %s or %s; '
                                'nothing is downloaded' % (e, data_dir, os.path.join(data_dir, 'MNIST', 'raw'))) from None
    if len(images) != len(labels):
        raise ValueError('%d test images but %d labels under %s' % (len(images), len(labels), data_dir))
    return images, labels


def generate(data_dir, seq_len, seed, digits, frame_size, max_speed, device, timings=None):
    """The four arrays of the reference's file, as host arrays: {'sequences', 'latents', 'labels', 'digits'}.  timings: optional dict that
    receives the seconds spent in 'read', 'draw', 'kernel' and 'download' (the device is then synchronised after the launch)."""
    device = require_gpu('Moving-MNIST test', device)
    t0 = time.perf_counter()
    images, labels = read_test_digits(data_dir)
    if digits < 1 or len(images) < digits:
        raise ValueError('%d digits per video need at least as many test images (found %d)' % (digits, len(images)))
    t1 = time.perf_counter()
    digits_idx, init = draw_test_set(len(images), images.shape[1:], frame_size, max_speed, digits, seed)
    t2 = time.perf_counter()
    frames, latents = ops.moving_mnist_testset(torch.from_numpy(images).to(device), init, seq_len, frame_size)
    if timings is not None:
        torch.cuda.synchronize(device)
    t3 = time.perf_counter()
    used = digits_idx[:init.shape[0] * digits]
    out = dict(sequences=frames.cpu().numpy(), latents=latents.cpu().numpy().astype(np.int64),
               labels=labels[used].reshape(-1, digits).astype(np.uint8), digits=images[used].reshape((-1, digits) + images.shape[1:]))
    if timings is not None:
        timings.update(read=t1 - t0, draw=t2 - t1, kernel=t3 - t2, download=time.perf_counter() - t3)
    return out


def build_parser():
    p = argparse.ArgumentParser(prog='Moving MNIST testing set generation.', formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                description='Generates the Moving MNIST testing set on an MI355X. Videos and latent space (position, speed) '
                                            'are saved in an npz file.')
    p.add_argument('--data_dir', type=str, metavar='DIR', required=True,
                   help='Folder that holds the raw MNIST test files and where the testing set will be saved.')
    p.add_argument('--seq_len', type=int, metavar='LEN', default=100, help='Number of frames per testing sequences.')
    p.add_argument('--seed', type=int, metavar='SEED', default=42, help='Fixed NumPy seed to produce the same dataset at each run.')
    p.add_argument('--digits', type=int, metavar='NUM', default=2, help='Number of digits to appear in each video.')
    p.add_argument('--frame_size', type=int, metavar='SIZE', default=64, help='Size of generated frames.')
    p.add_argument('--max_speed', type=int, metavar='SPEED', default=4, help='Maximum speed of generated trajectories.')
    p.add_argument('--device', type=int, metavar='DEVICE', default=None, help='GPU the generation runs on (required: there is no CPU mode).')
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.device is None:
        parser.error('the generation runs on an MI355X: pass --device N (there is no CPU mode)')
    arrays = generate(args.data_dir, args.seq_len, args.seed, args.digits, args.frame_size, args.max_speed, torch.device('cuda', args.device))
    fname = f'mmnist_test_{args.digits}digits_{args.frame_size}.npz'
    print(f'Saving testset at {os.path.join(args.data_dir, fname)}')
    if not os.path.isdir(args.data_dir):
        os.makedirs(args.data_dir)
    np.savez_compressed(os.path.join(args.data_dir, fname), **arrays)


if __name__ == '__main__':
    main()

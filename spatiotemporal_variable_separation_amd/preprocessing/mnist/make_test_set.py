"""Moving-MNIST test set generated on the device (reference: preprocessing/mnist/make_test_set.py, same flags plus --device):

    python -m spatiotemporal_variable_separation_amd.preprocessing.mnist.make_test_set --data_dir D --device 0 [--stochastic]

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

`--stochastic` (not in the reference, whose script always builds its sampler with deterministic=True) writes D/smmnist_test_*.npz, the file
`make_dataset(train=False, deterministic=False)` looks for: the same loop over a sampler that redraws the speed vector from the stream at
every bounce.  The trajectories then depend on the stream as they go, so the host draws only the permutation; one launch of one workgroup
walks all trajectories from the stream in HBM (ops.mmnist_stochastic_trajectories) and one launch renders them
(ops.moving_mnist_testset_place).  Same keys, dtypes and layouts, both compression routes; profiles/smnist_testset_timing.md.

Who compresses the file: the environment variable VARSEP_NPZ_COMPRESS=host|device (`save_test_set(..., compress=)` in code; the keyword
wins, then the variable, then the default `host`).  `host` is np.savez_compressed as above.  `device` keeps the four arrays in HBM
(`generate_device`), compresses them there (ops.deflate_raw_slabs: csrc/vs_deflate.hip, run matching + dynamic Huffman codes per 32 KiB
chunk; ops.crc32) and writes the compressed bytes into the same zip container (utils/npz.py); np.load and the reference's readers load
either file to the same arrays.  Measurements: profiles/deflate_timing.md.
"""
import argparse
import os
import time

import numpy as np
import torch

from ... import ops
from ..._lib import VarsepHipError, require_cuda
from ...utils.savez import COMPRESS_ENV, npz_compressor, savez_compressed  # noqa: F401  (the rule lives there; importable from here as before)
from ...data.device import require_gpu
from ...data.moving_mnist import draw_test_set, read_mnist_images, read_mnist_labels, stochastic_test_set


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


def _videos(images, seq_len, seed, digits, frame_size, max_speed, device, stochastic):
    """(digits_idx, n_videos, the images on the device, frames uint8 [T, N, 1, F, F], latents int32 [T, N, digits, 4], the time after the
    host's draws).  Deterministic: every draw on the host (`draw_test_set`), one launch.  Stochastic: the host draws the permutation only;
    one launch walks the trajectories from the stream in HBM and one renders them (`stochastic_test_set`)."""
    if digits < 1 or len(images) < digits:
        raise ValueError('%d digits per video need at least as many test images (found %d)' % (digits, len(images)))
    if stochastic:
        drawn = time.perf_counter()                 # the host's only draw, the permutation, happens inside: microseconds
        dev_images = torch.from_numpy(images).to(device)
        digits_idx, frames, latents = stochastic_test_set(dev_images, frame_size, max_speed, digits, seed, seq_len)
        return digits_idx, len(images) // digits, dev_images, frames, latents, drawn
    digits_idx, init = draw_test_set(len(images), images.shape[1:], frame_size, max_speed, digits, seed)
    drawn = time.perf_counter()
    dev_images = torch.from_numpy(images).to(device)
    frames, latents = ops.moving_mnist_testset(dev_images, init, seq_len, frame_size)
    return digits_idx, init.shape[0], dev_images, frames, latents, drawn


def generate(data_dir, seq_len, seed, digits, frame_size, max_speed, device, timings=None, stochastic=False):
    """The four arrays of the reference's file, as host arrays: {'sequences', 'latents', 'labels', 'digits'}.  timings: optional dict that
    receives the seconds spent in 'read', 'draw', 'kernel' and 'download' (the device is then synchronised after the launch).
    stochastic=True: the arrays of `smmnist_test_*.npz` (the speed vector is redrawn at every bounce)."""
    device = require_gpu('Moving-MNIST test', device)
    t0 = time.perf_counter()
    images, labels = read_test_digits(data_dir)
    t1 = time.perf_counter()
    digits_idx, n_videos, _, frames, latents, t2 = _videos(images, seq_len, seed, digits, frame_size, max_speed, device, stochastic)
    if timings is not None:
        torch.cuda.synchronize(device)
    t3 = time.perf_counter()
    used = digits_idx[:n_videos * digits]
    out = dict(sequences=frames.cpu().numpy(), latents=latents.cpu().numpy().astype(np.int64),
               labels=labels[used].reshape(-1, digits).astype(np.uint8), digits=images[used].reshape((-1, digits) + images.shape[1:]))
    if timings is not None:
        timings.update(read=t1 - t0, draw=t2 - t1, kernel=t3 - t2, download=time.perf_counter() - t3)
    return out


def generate_device(data_dir, seq_len, seed, digits, frame_size, max_speed, device, timings=None, stochastic=False):
    """`generate` with the four arrays left on the device, in the file's dtypes and layouts: sequences uint8 [T, N, 1, F, F], latents int64
    [T, N, digits, 4] (widened on the device), labels uint8 [N, digits], digits uint8 [N, digits, h, w] (both uploaded once).  timings:
    as in `generate`, without 'download'."""
    device = require_gpu('Moving-MNIST test', device)
    t0 = time.perf_counter()
    images, labels = read_test_digits(data_dir)
    t1 = time.perf_counter()
    digits_idx, n_videos, dev_images, frames, latents, t2 = _videos(images, seq_len, seed, digits, frame_size, max_speed, device, stochastic)
    used = torch.from_numpy(np.ascontiguousarray(digits_idx[:n_videos * digits]).astype(np.int64)).to(device)
    out = dict(sequences=frames, latents=latents.to(torch.int64),
               labels=torch.from_numpy(labels.astype(np.uint8)).to(device)[used].reshape(-1, digits).contiguous(),
               digits=dev_images[used].reshape((-1, digits) + tuple(images.shape[1:])).contiguous())
    if timings is not None:
        torch.cuda.synchronize(device)
        timings.update(read=t1 - t0, draw=t2 - t1, kernel=time.perf_counter() - t2)
    return out


def save_test_set(path, arrays, compress=None, timings=None):
    """Writes the four arrays (host arrays or device tensors, `generate` / `generate_device`) to the .npz file `path` through
    utils/savez.savez_compressed.  compress: 'host' (tensors are downloaded; np.savez_compressed), 'device' (device tensors are compressed
    in HBM and only the compressed bytes are downloaded: ops.deflate_raw_slabs, ops.crc32, utils/npz.write_npz) or None
    (`npz_compressor`).  Unlike the general writer, 'device' here takes device tensors only: the set was generated to stay in HBM.
    timings: optional dict that receives the seconds of 'download' + 'write' (host) or of 'write' (device: compression, download of the
    compressed bytes and file together)."""
    compress = npz_compressor(compress)
    if compress == 'device':
        for name, t in arrays.items():
            if not isinstance(t, torch.Tensor):
                raise VarsepHipError("save_test_set: compress='device' takes device tensors (generate_device); %s is a %s"
                                     % (name, type(t).__name__))
        require_cuda(*arrays.values())
    savez_compressed(path, arrays, compress, timings=timings)


def build_parser(stochastic=False):
    """The reference's flags plus --device; stochastic=True (the command line's parser, `main`) adds --stochastic, which the reference's
    script lacks (it always passes deterministic=True to its sampler)."""
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
    if stochastic:
        p.add_argument('--stochastic', action='store_true',
                       help='Generate the stochastic variant (the speed vector is redrawn at every bounce) and save it as smmnist_test_*.npz, '
                            'the file the dataset reads with deterministic=False.')
    return p


def file_name(digits, frame_size, stochastic=False):
    """`[s]mmnist_test_{digits}digits_{frame_size}.npz`: the name under which `MovingMNIST.make_dataset(train=False)` looks for the set."""
    return '%smmnist_test_%ddigits_%d.npz' % ('s' if stochastic else '', digits, frame_size)


def main(argv=None):
    parser = build_parser(stochastic=True)
    args = parser.parse_args(argv)
    if args.device is None:
        parser.error('the generation runs on an MI355X: pass --device N (there is no CPU mode)')
    compress = npz_compressor(None)
    make = generate_device if compress == 'device' else generate
    arrays = make(args.data_dir, args.seq_len, args.seed, args.digits, args.frame_size, args.max_speed, torch.device('cuda', args.device),
                  stochastic=args.stochastic)
    fname = file_name(args.digits, args.frame_size, args.stochastic)
    print(f'Saving testset at {os.path.join(args.data_dir, fname)}')
    if not os.path.isdir(args.data_dir):
        os.makedirs(args.data_dir)
    save_test_set(os.path.join(args.data_dir, fname), arrays, compress)


if __name__ == '__main__':
    main()

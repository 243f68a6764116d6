"""Inputs of the Moving-MNIST test-set fixture (tests/golden/mmnist_testset.npz), rebuilt bit for bit from seeds by the fixture generator
(tests/make_golden_mmnist_testset.py) and by the tests (tests/test_mmnist_testset_cpu.py, tests/test_mmnist_testset_gpu.py).  Nothing here
imports the reference.

A case is a run of the reference's preprocessing/mnist/make_test_set.py on `images` stand-in test digits (28 x 28 blobs built like those of
tests/eval_cli_inputs.py, with seeded labels): its flags --seed, --seq_len, --digits, --frame_size and --max_speed.
"""
import os

import numpy as np

from eval_cli_inputs import _digits

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'mmnist_testset.npz')
DIGIT = 28
ARRAYS = ('sequences', 'latents', 'labels', 'digits')

CASES = {
    'default': dict(images=24, seed=42, seq_len=20, digits=2, frame=64, speed=4, standin_seed=5101),     # the paper's geometry
    'fast3': dict(images=25, seed=7, seq_len=24, digits=3, frame=64, speed=9, standin_seed=5102),        # one image left over; several bounces per step
    'tight': dict(images=6, seed=3, seq_len=16, digits=1, frame=32, speed=4, standin_seed=5103),         # 4 pixels of room: a bounce nearly every frame
}
# A 28 x 28 digit in a 28 x 28 frame (x_max = 0, no room at all) cannot be a case: the reference's bounce loop (data/moving_mnist.py:201-251)
# does not terminate for a digit with a non-zero speed there -- each pass mirrors the position about the single allowed point (sx = dx ->
# -dx -> dx ...), so a collision is detected for ever.  make_golden_mmnist_testset.py shows this under a time limit (NO_ROOM below); the
# all-overlapping / 255-clip property of that geometry is tested with zero speeds against the restatement instead.
NO_ROOM = dict(images=8, seed=11, seq_len=8, digits=2, frame=28, speed=4, standin_seed=5104)


def standins(case):
    """(images uint8 [n, 28, 28], labels uint8 [n]) of a case (a name of CASES or a dict of its form)."""
    c = CASES[case] if isinstance(case, str) else case
    rng = np.random.RandomState(c['standin_seed'])
    images = _digits(c['images'], DIGIT, rng)
    labels = rng.randint(0, 10, size=c['images']).astype(np.uint8)
    return images, labels


def golden(case):
    """{'sequences', 'latents', 'labels', 'digits'} of a case as the reference wrote them."""
    with np.load(GOLDEN) as z:
        params = dict(zip(z['param_names'].tolist(), z[case + ':params'].tolist()))
        assert params == {k: CASES[case][k] for k in params}, (case, params)
        return {k: z[case + ':' + k] for k in ARRAYS}


def write_t10k(data_dir, images, labels, gz=False):
    """MNIST/raw/t10k-images-idx3-ubyte and t10k-labels-idx1-ubyte (plain or gzip) under `data_dir`."""
    import gzip
    raw = os.path.join(data_dir, 'MNIST', 'raw')
    os.makedirs(raw, exist_ok=True)
    opener, ext = (gzip.open, '.gz') if gz else (open, '')
    n, h, w = images.shape
    with opener(os.path.join(raw, 't10k-images-idx3-ubyte' + ext), 'wb') as f:
        f.write(np.array([2051, n, h, w], dtype='>i4').tobytes() + np.ascontiguousarray(images, dtype=np.uint8).tobytes())
    with opener(os.path.join(raw, 't10k-labels-idx1-ubyte' + ext), 'wb') as f:
        f.write(np.array([2049, n], dtype='>i4').tobytes() + np.ascontiguousarray(labels, dtype=np.uint8).tobytes())
    return data_dir

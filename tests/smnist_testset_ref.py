"""NumPy restatement of the reference's preprocessing/mnist/make_test_set.py run with a STOCHASTIC sampler (deterministic=False: the speed
vector is redrawn from the global stream at every bounce).  TEST INFRASTRUCTURE ONLY: the checker of `stochastic_test_set`
(data/moving_mnist.py), vs_moving_mnist_testset_place and the walk kernel's four-draw form.  Built on tests/smnist_ref.py, the restatement
of the sampler that tests/make_golden_smnist.py pins to the reference.

Pinned: tests/make_golden_smnist_testset.py runs the reference's own script on the stand-in digits and requires this file to reproduce all
four arrays and the final words of the global stream, for every case, before it writes tests/golden/smnist_testset.npz.

Follows make_test_set.py: the seed (:52), the permutation (:56), per video and digit `_compute_trajectory` (:74 -> data/moving_mnist.py:
154-170: four draws, then bounce with redraws / record the rounded position and the speed / move), compositing in float32 with the clip
at 255 (:78-83), the transpositions to time-major (:88-89).
"""
import numpy as np

import smnist_ref
from mmnist_draws_inputs import state_words


def walk_all(n_videos, digits, seq_len, frame, digit_shape, speed, note=None):
    """latents int64 [n_videos, digits, seq_len, 4] from the GLOBAL stream as it stands: per video and digit the four prefix draws and
    the walk."""
    x_max, y_max = frame - digit_shape[0], frame - digit_shape[1]
    cols = [(0, x_max + 1), (0, y_max + 1), (-speed, speed + 1), (-speed, speed + 1)]
    _, traj = smnist_ref.sample(np.random.randint, n_videos * digits, seq_len, cols, x_max, y_max, speed, note=note)
    return np.asarray(traj, dtype=np.int64).reshape(n_videos, digits, seq_len, 4)


def render(images, digit_idx, latents, frame):
    """sequences uint8 [T, N, 1, F, F] of the digits `digit_idx` [N, digits] at the positions of `latents` [N, digits, T, 4]."""
    n_videos, digits, seq_len = latents.shape[:3]
    h, w = images.shape[1:]
    videos = []
    for i in range(n_videos):
        x = np.zeros((seq_len, 1, frame, frame), dtype=np.float32)
        for n in range(digits):
            img = images[digit_idx[i, n]]
            for t in range(seq_len):
                sx, sy = latents[i, n, t, :2]
                x[t, 0, sx:sx + h, sy:sy + w] += img
        x[x > 255] = 255
        videos.append(x.astype(np.uint8))
    return np.array(videos, dtype=np.uint8).transpose(1, 0, 2, 3, 4)


def make_test_set(images, labels, seed, seq_len, digits, frame, speed, note=None):
    """({'sequences', 'latents', 'labels', 'digits'} as the script saves them, the words of the global stream after it).  The global stream is
    reseeded and left where the script leaves it, as the reference does."""
    np.random.seed(seed)
    digits_idx = np.random.permutation(len(images))
    n_videos = len(images) // digits
    latents = walk_all(n_videos, digits, seq_len, frame, images.shape[1:], speed, note)
    used = digits_idx[:n_videos * digits]
    arrays = dict(sequences=render(images, used.reshape(n_videos, digits), latents, frame), latents=latents.transpose(2, 0, 1, 3).astype(np.int64),
                  labels=labels[used].reshape(-1, digits).astype(np.uint8), digits=images[used].reshape((-1, digits) + images.shape[1:]))
    return arrays, state_words(np.random)

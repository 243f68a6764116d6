"""NumPy restatement of the reference's preprocessing/mnist/make_test_set.py (TEST INFRASTRUCTURE ONLY: the checker of
vs_moving_mnist_testset and of data/moving_mnist.py's `draw_test_set`), built on `oracle.mmnist_ref.process_collision`.

Pinned: tests/make_golden_mmnist_testset.py runs the reference's own script on the stand-in digits of tests/mmnist_testset_inputs.py and
requires this restatement to reproduce all four arrays of every case bit for bit before it writes tests/golden/mmnist_testset.npz;
tests/test_mmnist_testset_cpu.py replays the fixture against this file.

Follows make_test_set.py: the seed (:52), the permutation (:56), per video and digit `_compute_trajectory` (:74 -> data/moving_mnist.py:
154-170: four draws, then bounce / record the rounded position and the speed / move), compositing in float32 with the clip at 255 (:78-83),
the transpositions to time-major (:88-89).
"""
import numpy as np

from oracle.mmnist_ref import process_collision


def trajectory(sx, sy, dx, dy, seq_len, x_max, y_max):
    """[(rounded row, rounded column, row speed, column speed)] * seq_len from a start position and speed (moving_mnist.py:161-170)."""
    sx, sy, dx, dy = int(sx), int(sy), int(dx), int(dy)
    out = []
    for _ in range(seq_len):
        sx, sy, dx, dy = process_collision(sx, sy, dx, dy, x_max, y_max)
        out.append([int(round(sx)), int(round(sy)), dx, dy])
        sy += dy
        sx += dx
    return out


def draw(n_images, digit_shape, frame, speed, digits, seed):
    """(digits_idx, init int32 [n_images // digits, digits, 5]): the script's draws from the global stream, which is reseeded."""
    h, w = digit_shape
    np.random.seed(seed)
    digits_idx = np.random.permutation(n_images)
    init = np.empty((n_images // digits, digits, 5), dtype=np.int32)
    for i in range(n_images // digits):
        for n in range(digits):
            init[i, n, 0] = digits_idx[i * digits + n]
            init[i, n, 1] = np.random.randint(0, frame - h + 1)
            init[i, n, 2] = np.random.randint(0, frame - w + 1)
            init[i, n, 3] = np.random.randint(-speed, speed + 1)
            init[i, n, 4] = np.random.randint(-speed, speed + 1)
    return digits_idx, init


def render(images, init, seq_len, frame):
    """(sequences uint8 [T, N, 1, F, F], latents int64 [T, N, digits, 4]) of the videos described by `init`."""
    n_videos, digits = init.shape[0], init.shape[1]
    h, w = images.shape[1:]
    videos, latents = [], []
    for i in range(n_videos):
        x = np.zeros((seq_len, 1, frame, frame), dtype=np.float32)
        lat = []
        for n in range(digits):
            img = images[init[i, n, 0]]
            traj = trajectory(init[i, n, 1], init[i, n, 2], init[i, n, 3], init[i, n, 4], seq_len, frame - h, frame - w)
            lat.append(np.array(traj))
            for t in range(seq_len):
                sx, sy, _, _ = traj[t]
                x[t, 0, sx:sx + h, sy:sy + w] += img
        x[x > 255] = 255
        videos.append(x.astype(np.uint8))
        latents.append(np.array(lat))
    return np.array(videos, dtype=np.uint8).transpose(1, 0, 2, 3, 4), np.array(latents).transpose(2, 0, 1, 3).astype(np.int64)


def make_test_set(images, labels, seed, seq_len, digits, frame, speed):
    """{'sequences', 'latents', 'labels', 'digits'} as make_test_set.py saves them."""
    digits_idx, init = draw(len(images), images.shape[1:], frame, speed, digits, seed)
    sequences, latents = render(images, init, seq_len, frame)
    used = digits_idx[:init.shape[0] * digits]
    return dict(sequences=sequences, latents=latents, labels=labels[used].reshape(-1, digits).astype(np.uint8),
                digits=images[used].reshape((-1, digits) + images.shape[1:]))

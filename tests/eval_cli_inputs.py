"""Inputs of the evaluation-CLI fixtures (tests/golden/eval_cli_*), rebuilt bit for bit from seeds by the fixture generator
(tests/make_golden_eval_cli.py) and by the GPU tests (tests/test_eval_cli_gpu.py).  Nothing here imports the reference.

* Moving MNIST: raw MNIST idx files (train and t10k; 10 000 test digits, the count `SwapDataset` indexes) and an
  `mmnist_test_2digits_64.npz` whose `latents` hold 5 000 trajectories of valid positions and whose `sequences` hold a few test videos
  rendered along the first trajectories.
* WaveEq: simulation files and a pixel table in the layout of oracle/wave_data_ref.write_fixture_set, with the frame height equal to
  the number of frames after downsampling (the reference's `__len__` counts windows with the frame height, wave_eq.py:62-65).
"""
import json
import os
import re

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')

MNIST = dict(n_train=512, n_test=10000, n_traj=5000, n_videos=8, n_frames=16, n_object=2, frame=64, digit=28, seed=2024)
# nt_cond of tests/golden/ckpt_dcgan_tiny.  test.py runs with --batch_size 3 (8 videos: a ragged last batch); test_disentanglement.py
# with 4, because the reference fails on a ragged batch there
MNIST_RUN = dict(nt_pred=10, batch_size={'test': 3, 'test_disentanglement': 4}, test_seed=1)
MNIST_PARAMS = dict(architecture='dcgan', data='mnist', n_object=2, nt_cond=3, nt_pred=4, offset=3, skipco=False)

WAVE = dict(n_files=10, nt_raw=92, downsample=2, H=46, W=6, n_pixels=10, seed=77)
WAVE_RUN = dict(batch_size=4)
WAVE_PARAMS = {
    'wave': dict(architecture='mlp', data='wave', nt_cond=4, nt_pred=10, offset=4, downsample=2, n_wave_points=10, skipco=False),
    'wave_partial': dict(architecture='mlp', data='wave_partial', nt_cond=3, nt_pred=10, offset=0, downsample=2, n_wave_points=10,
                         skipco=False),
}


def _digits(n, size, rng):
    """uint8 [n, size, size] digit-like blobs: 1-3 soft strokes each."""
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float32)
    img = np.zeros((n, size, size), dtype=np.float32)
    for _ in range(3):
        keep = rng.uniform(size=n) < 0.8
        cy, cx = rng.uniform(6, size - 6, size=(2, n)).astype(np.float32)
        ang = rng.uniform(0, np.pi, size=n).astype(np.float32)
        length = rng.uniform(4, 10, size=n).astype(np.float32)
        width = rng.uniform(1.0, 2.2, size=n).astype(np.float32)
        dy, dx = np.sin(ang)[:, None, None], np.cos(ang)[:, None, None]
        along = (yy - cy[:, None, None]) * dy + (xx - cx[:, None, None]) * dx
        across = -(yy - cy[:, None, None]) * dx + (xx - cx[:, None, None]) * dy
        img += keep[:, None, None] * np.exp(-(across / width[:, None, None]) ** 2) * (np.abs(along) <= length[:, None, None])
    return (np.clip(img, 0, 1) * 255.0).astype(np.uint8)


def _write_idx(path, images):
    n, h, w = images.shape
    with open(path, 'wb') as f:
        f.write(np.array([2051, n, h, w], dtype='>i4').tobytes())
        f.write(np.ascontiguousarray(images, dtype=np.uint8).tobytes())


def read_idx(path):
    with open(path, 'rb') as f:
        raw = f.read()
    _, n, h, w = np.frombuffer(raw[:16], dtype='>i4')
    return np.frombuffer(raw, dtype=np.uint8, offset=16).reshape(int(n), int(h), int(w)).copy()


def _trajectories(n_frames, n_seq, n_object, room, rng):
    """int64 [n_frames, n_seq, n_object, 4] = (sx, sy, dx, dy): straight moves reflected at 0 and `room`."""
    pos = rng.randint(0, room + 1, size=(n_seq, n_object, 2)).astype(np.int64)
    vel = rng.randint(-4, 5, size=(n_seq, n_object, 2)).astype(np.int64)
    out = np.empty((n_frames, n_seq, n_object, 4), dtype=np.int64)
    for t in range(n_frames):
        out[t, ..., :2], out[t, ..., 2:] = pos, vel
        pos = pos + vel
        low, high = pos < 0, pos > room
        pos = np.where(low, -pos, np.where(high, 2 * room - pos, pos))
        vel = np.where(low | high, -vel, vel)
    return out


def write_mnist_inputs(data_dir):
    """MNIST/raw/{train,t10k}-images-idx3-ubyte and mmnist_test_2digits_64.npz under `data_dir`."""
    m = MNIST
    rng = np.random.RandomState(m['seed'])
    raw = os.path.join(data_dir, 'MNIST', 'raw')
    os.makedirs(raw, exist_ok=True)
    train = _digits(m['n_train'], m['digit'], rng)
    test = _digits(m['n_test'], m['digit'], rng)
    _write_idx(os.path.join(raw, 'train-images-idx3-ubyte'), train)
    _write_idx(os.path.join(raw, 't10k-images-idx3-ubyte'), test)
    latents = _trajectories(m['n_frames'], m['n_traj'], m['n_object'], m['frame'] - m['digit'], rng)
    seq = np.zeros((m['n_frames'], m['n_videos'], 1, m['frame'], m['frame']), dtype=np.float32)
    picks = rng.randint(0, m['n_test'], size=(m['n_videos'], m['n_object']))
    d = m['digit']
    for t in range(m['n_frames']):
        for v in range(m['n_videos']):
            for i in range(m['n_object']):
                sx, sy = latents[t, v, i, :2]
                seq[t, v, 0, sx:sx + d, sy:sy + d] += test[picks[v, i]]
    seq = np.minimum(seq, 255).astype(np.uint8)
    np.savez(os.path.join(data_dir, 'mmnist_test_%ddigits_%d.npz' % (m['n_object'], m['frame'])), sequences=seq, latents=latents)
    return data_dir


def write_wave_inputs(data_dir):
    """data/wave_<i>.pt simulations and pixels/pixels.npz under `data_dir` (which must be digit-free: the reference's train/test
    split reads the first integer of the whole path)."""
    assert not re.findall(r'\d', data_dir), 'WaveEq fixture directory must be digit-free: %s' % data_dir
    w = WAVE
    g = torch.Generator().manual_seed(w['seed'])
    os.makedirs(os.path.join(data_dir, 'data'), exist_ok=True)
    os.makedirs(os.path.join(data_dir, 'pixels'), exist_ok=True)
    t = torch.arange(w['nt_raw'], dtype=torch.float32)[:, None, None]
    yy = torch.arange(w['H'], dtype=torch.float32)[None, :, None]
    xx = torch.arange(w['W'], dtype=torch.float32)[None, None, :]
    for i in range(w['n_files']):
        k = torch.rand(3, generator=g)
        sim = torch.sin(0.2 * (1 + k[0]) * yy - 0.15 * (1 + k[1]) * t) * torch.cos(0.5 * xx + k[2] * t * 0.1) \
            + 0.05 * torch.rand((w['nt_raw'], w['H'], w['W']), generator=g)
        torch.save({'simul': sim * (1.0 + i)}, os.path.join(data_dir, 'data', 'wave_%d.pt' % i))
    rng = np.random.RandomState(w['seed'])
    np.savez(os.path.join(data_dir, 'pixels', 'pixels.npz'), rand_w=rng.randint(0, w['H'], size=32),
             rand_h=rng.randint(0, w['W'], size=32))
    return data_dir


def write_params(xp_dir, params):
    os.makedirs(xp_dir, exist_ok=True)
    with open(os.path.join(xp_dir, 'params.json'), 'w') as f:
        json.dump(params, f, indent=4, sort_keys=True)


def parse_results(stdout):
    """{name: value} of the lines after `Results:` (test/mnist/*.py) and of `MSE at t+40: ...` (test/wave/test.py)."""
    out, on = {}, False
    for line in stdout.splitlines():
        if line.startswith('MSE at t+40:'):
            out['mse_t40'] = float(line.split(':', 1)[1])
        if line.strip() == 'Results:':
            on = True
            continue
        parts = line.split()
        if on and len(parts) == 2:
            try:
                out[parts[0]] = float(parts[1])
            except ValueError:
                pass
    return out

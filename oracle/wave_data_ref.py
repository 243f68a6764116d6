"""CPU restatement of the reference's WaveEq datasets (TEST INFRASTRUCTURE ONLY -- see oracle/__init__.py).

Follows var_sep/data/wave_eq.py line by line in plain torch on the host; pinned to the reference itself by
tests/golden/wave_loader.npz (oracle/make_golden_data.py runs the real `WaveEq` / `WaveEqPartial` behind a seeded
`DataLoader(shuffle=True)`).  The product (spatiotemporal_variable_separation_amd/data/wave_eq.py) keeps the set in HBM and
gathers batches with a HIP kernel; the GPU tests compare it with this file and with the golden batches.
"""
import os
import re

import numpy as np
import torch
from torch.utils.data import Dataset


def extract_id(string):                                              # wave_eq.py:25-26
    return int(re.findall(r'\d+', string)[0])


class WaveEqRef(Dataset):
    def __init__(self, data_dir, nt_cond, seq_len, train, downsample):  # wave_eq.py:30-62
        self.nt_cond, self.seq_len = nt_cond, seq_len
        base_path = os.path.join(data_dir, 'data')
        files = [os.path.join(base_path, f) for f in os.listdir(base_path)]
        max_seq = int(0.8 * len(files))
        files = [f for f in files if (extract_id(f) < max_seq) == bool(train)]
        self.size = len(files)
        self.all_data = []
        data = None
        for file in files:
            data = torch.load(file).get('simul')
            max_, min_ = data.max(), data.min()
            data = (data - min_) / (max_ - min_)
            data = data[::downsample]
            self.nt = len(data)
            self.all_data.append(data)
        self.full_seq_len = data[0].size(0)                          # wave_eq.py:62 (frame height)

    def __len__(self):                                               # wave_eq.py:64-65
        return self.size * (self.full_seq_len - self.seq_len + 1)

    def __getitem__(self, idx):                                      # wave_eq.py:67-72
        idx_seq = idx // (self.nt + 1 - self.seq_len)
        idx_in_seq = idx % (self.nt + 1 - self.seq_len)
        full_state = self.all_data[idx_seq][idx_in_seq: idx_in_seq + self.seq_len].unsqueeze(1)
        return full_state[:self.nt_cond], full_state[self.nt_cond: self.seq_len]


class WaveEqPartialRef(WaveEqRef):
    def __init__(self, data_dir, nt_cond, seq_len, train, downsample, n_pixels):   # wave_eq.py:77-84
        super().__init__(data_dir, nt_cond, seq_len, train, downsample)
        pixels = np.load(os.path.join(data_dir, 'pixels', 'pixels.npz'), allow_pickle=True)
        self.rand_w, self.rand_h, self.n_wave_points = pixels['rand_w'], pixels['rand_h'], n_pixels

    def __getitem__(self, idx):                                      # wave_eq.py:86-90
        cond, target = super().__getitem__(idx)
        cond = cond[:, :, self.rand_w[:self.n_wave_points], self.rand_h[:self.n_wave_points]]
        target = target[:, :, self.rand_w[:self.n_wave_points], self.rand_h[:self.n_wave_points]]
        return cond, target


# ---- the fixture set shared by the generator and the tests ---------------------------------------------------------------------
FIXTURE = dict(n_files=10, nt_raw=36, H=12, W=10, downsample=2, nt_cond=3, seq_len=7, n_pixels=9, batch_size=5, seed=4321)


def write_fixture_set(data_dir):
    """Deterministic simulation files + pixel table under `data_dir` (which must not contain digits: the reference's split reads
    the first integer of the whole path)."""
    from oracle.detdata import det_uniform
    assert not re.findall(r'\d', data_dir), 'fixture directory must be digit-free: %s' % data_dir
    f = FIXTURE
    os.makedirs(os.path.join(data_dir, 'data'), exist_ok=True)
    os.makedirs(os.path.join(data_dir, 'pixels'), exist_ok=True)
    for i in range(f['n_files']):
        sim = det_uniform((f['nt_raw'], f['H'], f['W']), 100 + i) * (1.0 + i) - 0.25 * i
        torch.save({'simul': sim.clone()}, os.path.join(data_dir, 'data', 'wave_%d.pt' % i))
    rng = np.random.RandomState(7)
    np.savez(os.path.join(data_dir, 'pixels', 'pixels.npz'), rand_w=rng.randint(0, f['H'], size=32), rand_h=rng.randint(0, f['W'], size=32))


class sorted_listdir:
    """The reference takes the files in `os.listdir` order (wave_eq.py:40), which depends on the file system; the golden batches
    are recorded -- and replayed -- under a sorted listing so that they mean the same thing on every machine."""

    def __enter__(self):
        self._real = os.listdir
        os.listdir = lambda path='.': sorted(self._real(path))
        return self

    def __exit__(self, *exc):
        os.listdir = self._real
        return False


def fixture_dir():
    """A directory of this process alone, directly under the temporary directory (a shared parent would belong to whichever user
    created it first); user and process id are spelt in letters: the path holds no digit."""
    import tempfile
    tmp = tempfile.gettempdir()
    if re.findall(r'\d', tmp):
        tmp = '/tmp'
    suffix = ''.join(chr(ord('a') + (n // 26 ** k) % 26) for n in (os.getuid(), os.getpid()) for k in range(6))
    return os.path.join(tmp, 'varsep_wave_fixture_' + suffix)

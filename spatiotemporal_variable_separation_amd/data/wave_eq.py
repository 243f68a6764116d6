"""WaveEq datasets resident in HBM, batches assembled on the device (reference: var_sep/data/wave_eq.py:29-90).

The reference keeps the normalised simulations in host memory and lets a DataLoader slice one window per item and stack them.
At this path's step rate (128 sequences x 25 frames x 16 KB per 1.8 ms = 29 GB/s) no host loader keeps up, and the whole
set is small next to 288 GB of HBM: here the simulations live on the GPU as one [n_seq, nt, H*W] fp32 tensor and a batch is
ONE gather launch (`vs_gather_windows`) driven by the sampler's item indices.  Item numbering, file selection,
normalisation and the pixel subset of `WaveEqPartial` follow the reference line by line -- including its two quirks: the
train/test split reads the first integer of the file's FULL PATH (wave_eq.py:25-26, 43-46), and `__len__` counts
windows with the frame HEIGHT where `__getitem__` uses the sequence length (wave_eq.py:62-65) -- so that a seeded sampler
visits the same windows in the same order.  `DeviceBatchLoader` (data/device.py) replaces `DataLoader(dataset, shuffle=True)` (main.py:113):
the index stream comes from torch's own RandomSampler / BatchSampler, only the 4-byte indices cross PCIe.
"""
import os
import re

import numpy as np
import torch

from .. import ops
from .device import DeviceSet, require_gpu


def extract_id(string):
    """First run of digits of the string (wave_eq.py:25-26) -- applied to the joined path, like the reference."""
    return int(re.findall(r'\d+', string)[0])


class WaveEq(DeviceSet):
    """`WaveEq(data_dir, nt_cond, seq_len, train, downsample)` (wave_eq.py:29-72) with the data on `device`."""

    def __init__(self, data_dir, nt_cond, seq_len, train, downsample, device=None):
        self.nt_cond, self.seq_len, self.train, self.downsample = nt_cond, seq_len, train, downsample
        device = require_gpu('WaveEq', device, hint=' (tests use oracle/wave_data_ref.py for CPU results)')
        base_path = os.path.join(data_dir, 'data')
        files = [os.path.join(base_path, f) for f in os.listdir(base_path)]
        max_seq = int(0.8 * len(files))
        files = [f for f in files if (extract_id(f) < max_seq) == bool(train)]
        sims = []
        for file in files:
            data = torch.load(file).get('simul')
            max_, min_ = data.max(), data.min()
            data = (data - min_) / (max_ - min_)                    # per-file min-max (wave_eq.py:55-57), on the host in fp32
            sims.append(data[::downsample])
        if not sims:
            raise ValueError('no simulation files selected in %s' % base_path)
        if any(s.shape != sims[0].shape for s in sims):
            raise ValueError('the simulations must share one [nt, H, W] shape to live in one HBM tensor')
        self._install(torch.stack(sims), device)

    def _install(self, sims, device):
        """sims: the normalised, downsampled simulations of this half of the set, fp32 [size, nt, H, W] on the host or on `device`."""
        self.size, self.nt = sims.shape[0], sims.shape[1]
        self.full_seq_len = sims.shape[2]                            # wave_eq.py:62: the frame height, not nt
        self.frame_shape = tuple(sims.shape[2:])
        self.all_data = sims.reshape(self.size, self.nt, -1).to(device).contiguous()
        self.windows_per_seq = self.nt + 1 - self.seq_len            # wave_eq.py:69-70
        if self.windows_per_seq < 1:
            raise ValueError('seq_len %d exceeds the %d frames of a simulation' % (self.seq_len, self.nt))
        self._pixels = None

    @classmethod
    def simulated(cls, nt_cond, seq_len, train, downsample, size=300, sim_len=300, seed=42, dt=0.001, device=None, **extra):
        """The set `gen_wave --size --seq_len sim_len --seed --dt` would write and `cls(data_dir, ...)` would read back, without the files:
        one vs_wave_simulate launch draws the reference's parameters (preprocessing/wave/gen_wave.py: wave_parameters), simulates every
        sequence and normalises it with its own minimum and maximum, (x - min) / (max - min) in fp32 as the file route does on the host;
        sequences below int(0.8 * size) are the training half, the others the test half.  Only the parameter table crosses PCIe."""
        from ..preprocessing.wave.gen_wave import simulate
        self = cls.__new__(cls)
        self.nt_cond, self.seq_len, self.train, self.downsample = nt_cond, seq_len, train, downsample
        device = require_gpu(cls.__name__, device)
        sims, _, self.velocities = simulate(size, sim_len, seed, dt, device, normalise=True)
        max_seq = int(0.8 * size)
        sims = sims[:max_seq] if train else sims[max_seq:]
        if sims.shape[0] == 0:
            raise ValueError('no simulation falls into the %s half of a set of %d' % ('training' if train else 'test', size))
        self.velocities = self.velocities[:max_seq] if train else self.velocities[max_seq:]
        self._install(sims[:, ::downsample], device)
        self._simulated_extra(**extra)
        return self

    def _simulated_extra(self):
        pass

    def __len__(self):
        return self.size * (self.full_seq_len - self.seq_len + 1)

    def _check(self, idx_max):
        if idx_max >= self.size * self.windows_per_seq:
            raise IndexError('item %d is outside the %d windows of the set' % (idx_max, self.size * self.windows_per_seq))

    def batch(self, item_idx, out_dtype=torch.float32):
        """item_idx: int32 device tensor [B] (or a list of ints) -> (cond [B, nt_cond, 1, ...], target [B, seq_len-nt_cond, 1, ...])."""
        if not isinstance(item_idx, torch.Tensor):
            self._check(max(item_idx))
            item_idx = torch.tensor(list(item_idx), dtype=torch.int32).to(self.all_data.device, non_blocking=True)
        x = ops.gather_windows(self.all_data, item_idx, self.windows_per_seq, self.seq_len, self._pixels, out_dtype)
        tail = (self._pixels.numel(),) if self._pixels is not None else self.frame_shape
        x = x.view((x.shape[0], self.seq_len, 1) + tuple(tail))
        return x[:, :self.nt_cond], x[:, self.nt_cond:]


class WaveEqPartial(WaveEq):
    """`WaveEqPartial(..., n_pixels)` (wave_eq.py:75-90): every frame reduced to n_pixels fixed (row, column) positions."""

    def __init__(self, data_dir, nt_cond, seq_len, train, downsample, n_pixels, device=None):
        super().__init__(data_dir, nt_cond, seq_len, train, downsample, device=device)
        pixels = np.load(os.path.join(data_dir, 'pixels', 'pixels.npz'), allow_pickle=True)
        self._install_pixels(pixels['rand_w'], pixels['rand_h'], n_pixels)

    def _install_pixels(self, rand_w, rand_h, n_pixels):
        self.rand_w, self.rand_h = rand_w, rand_h
        self.n_wave_points = n_pixels
        H, W = self.frame_shape
        rows = np.asarray(self.rand_w[:n_pixels]).astype(np.int64)
        cols = np.asarray(self.rand_h[:n_pixels]).astype(np.int64)
        rows = np.where(rows < 0, rows + H, rows)                    # numpy-style negative indices, as advanced indexing allows
        cols = np.where(cols < 0, cols + W, cols)
        if rows.size and (rows.max() >= H or cols.max() >= W):
            raise IndexError('pixel table addresses positions outside the %dx%d frames' % (H, W))
        self._pixels = torch.from_numpy((rows * W + cols).astype(np.int32)).to(self.all_data.device)

    @classmethod
    def simulated(cls, nt_cond, seq_len, train, downsample, n_pixels, size=300, sim_len=300, seed=42, dt=0.001, pixel_seed=42, n_drawn=100,
                  device=None):
        """`WaveEq.simulated` reduced to `n_pixels` positions of the table `gen_pixels --number n_drawn --seed pixel_seed` would write."""
        return super().simulated(nt_cond, seq_len, train, downsample, size=size, sim_len=sim_len, seed=seed, dt=dt, device=device,
                                 n_pixels=n_pixels, pixel_seed=pixel_seed, n_drawn=n_drawn)

    def _simulated_extra(self, n_pixels, pixel_seed, n_drawn):
        from ..preprocessing.wave.gen_pixels import draw_pixels
        self._install_pixels(*draw_pixels(n_drawn, self.frame_shape[0], pixel_seed), n_pixels)

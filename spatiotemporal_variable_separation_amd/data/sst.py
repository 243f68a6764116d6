"""SST (sea-surface temperature) zones resident in HBM, batches gathered on the device (reference: var_sep/data/sst.py:24-99).

The reference keeps one normalised [L, 64, 64] array per zone on the host and slices `nt_cond + nt_pred` consecutive days per item; a
DataLoader stacks the items.  Here the normalised days of all zones live in HBM once as one fp32 [Z * L, 4096] timeline, an item is an
entry of an int32 table -- the index of its first day -- and a batch is one forward gather launch (`vs_gather_timeline`, step +1) driven by
the sampler's item indices.  For evaluation the per-day constants (the spatial mean / std of the normalisation and the climatology) and the
per-zone range sit beside the frames, and a batch also names, per row, the day of its first target frame and its zone: that is all
`vs_sst_frame_metrics` needs to undo the normalisation on the device.

Everything before the upload is `build_zones`, a pure NumPy function that needs no GPU and no hard netCDF4 dependency.  It follows the
reference's `_normalize` line by line, in the dtype NumPy's promotion gives each zone (a float64 `daily_mean` makes the zone float64, a
float32 one keeps it float32), and rounds once to fp32 at the end, as `__getitem__` does.  Two documented divergences: zones of unequal
length raise ValueError (the reference keeps the last zone's length and would index the others wrongly), and so does a half too short to
hold one window.
"""
import os

import numpy as np
import torch

from .device import TimelineSet, read_optional, require_gpu

VAR_NAMES = ('thetao', 'daily_mean', 'daily_std')
NC_NAME = 'data_{}.nc'
NPZ_NAME = 'data_{}.npz'
ZONE_SIZE = 64
CONVERSION_HINT = ("import netCDF4, numpy as np; v = netCDF4.Dataset('{nc}', 'r').variables\n"
                   "np.savez('{npz}', thetao=v['thetao'][:].data, daily_mean=v['daily_mean'][:].data, daily_std=v['daily_std'][:].data)")


def extract_data(data_dir, zone):
    """{name: array} of one zone: `data_{zone}.nc` through netCDF4 when that module imports and the file exists -- the raw `.data` of the
    masked arrays, as sst.py:24-29 takes it -- else `data_{zone}.npz` with the same three arrays under the same names."""
    def read_nc(netCDF4, path):
        loaded_file = netCDF4.Dataset(path, 'r')
        return {var: np.asarray(loaded_file.variables[var][:].data) for var in VAR_NAMES}

    return read_optional('netCDF4', os.path.join(data_dir, NC_NAME.format(zone)), os.path.join(data_dir, NPZ_NAME.format(zone)),
                         read_nc, lambda z: {var: z[var] for var in VAR_NAMES}, 'zone',
                         CONVERSION_HINT.format(nc=NC_NAME.format(zone), npz=NPZ_NAME.format(zone)))


def build_zones(data_dir, zones):
    """Host half of `SST._normalize` (sst.py:64-78) and of the evaluation script's `get_min` (test/sst/test.py:29-34), NumPy only ->
    (frames, consts, zone_range, L):
      frames      fp32 [Z * L, 64 * 64]: per zone, in the order given, the climatology removed, then the per-day spatial z-score; computed in
                  the dtype NumPy gives the reference's expressions and rounded ONCE to fp32;
      consts      fp32 [Z * L, 4] = (mu_norm, std_norm, mu_clim, std_clim) per day, each rounded to fp32 as the script's `torch.tensor(...,
                  dtype=torch.float)` does;
      zone_range  fp32 [Z, 2] = (min, max) of the normalised zone, taken BEFORE the fp32 rounding, then rounded;
      L           days per zone (the same for every zone, else ValueError)."""
    zones = list(zones)
    if not zones:
        raise ValueError('no SST zone was named')
    frames, consts, zone_range, L = [], [], [], None
    for zone in zones:
        zdata = extract_data(data_dir, zone)
        thetao = zdata['thetao']
        if thetao.ndim != 3 or len(zdata['daily_mean']) != len(thetao) or len(zdata['daily_std']) != len(thetao):
            raise ValueError('zone %s: thetao [L, H, W] with daily_mean [L] and daily_std [L] expected (got %s, %s, %s)'
                             % (zone, thetao.shape, zdata['daily_mean'].shape, zdata['daily_std'].shape))
        if L is None:
            L = len(thetao)
        elif len(thetao) != L:
            raise ValueError('zone %s holds %d days, the zones before it %d: zones of unequal length cannot share one item index'
                             % (zone, len(thetao), L))
        climate_mean, climate_std = zdata['daily_mean'].reshape(-1, 1, 1), zdata['daily_std'].reshape(-1, 1, 1)
        thetao = (thetao - climate_mean) / climate_std
        mean = thetao.mean(axis=(1, 2)).reshape(-1, 1, 1)
        std = thetao.std(axis=(1, 2)).reshape(-1, 1, 1)
        thetao = (thetao - mean) / std
        zone_range.append([np.float32(thetao.min()), np.float32(thetao.max())])
        frames.append(thetao.astype(np.float32).reshape(L, -1))
        consts.append(np.stack([np.asarray(c).reshape(-1).astype(np.float32) for c in (mean, std, climate_mean, climate_std)], axis=1))
    if len(zones) * L >= 2 ** 31:
        raise ValueError('%d days do not fit the int32 item table' % (len(zones) * L))
    return (np.ascontiguousarray(np.concatenate(frames, axis=0)), np.ascontiguousarray(np.concatenate(consts, axis=0)),
            np.asarray(zone_range, dtype=np.float32).reshape(len(zones), 2), L)


def half_bounds(L, nt_cond, nt_pred, train):
    """(first_, len_) of sst.py:53-61: the train half starts at day 0 and counts int(0.8 L) days, the test half starts at int(0.8 L) and
    counts the rest; each loses nt_pred + nt_cond + 1 items.  ValueError when no window is left."""
    first_ = 0 if train else int(0.8 * L)
    len_ = int(0.8 * L) if train else L - int(0.8 * L)
    len_ = len_ - nt_pred - nt_cond - 1
    if nt_cond < 1 or nt_pred < 0 or len_ < 1:
        raise ValueError('the %s half of %d days is too short to hold one window of %d + %d days' % ('train' if train else 'test', L, nt_cond, nt_pred))
    return first_, len_


def item_table(n_zones, L, nt_cond, nt_pred, train):
    """int32 [n_zones * len_]: the first day, in the [Z * L] timeline, of every item.  Item i lies in zone i // len_; the reference's
    `idx_id = i % len_ + nt_cond + 1 + first_` is the LAST conditioning day (sst.py:83-89), so the window starts at i % len_ + first_ + 2."""
    first_, len_ = half_bounds(L, nt_cond, nt_pred, train)
    table = (np.arange(n_zones, dtype=np.int64)[:, None] * L + np.arange(len_, dtype=np.int64)[None] + first_ + 2).reshape(-1)
    assert table.max() + nt_cond + nt_pred <= n_zones * L
    return table.astype(np.int32), len_


class SST(TimelineSet):
    """One half (train or test) of the SST windows of `zones`, with the reference's signature plus `device`.  Items are
    (cond [nt_cond, 1, 64, 64], target [nt_pred, 1, 64, 64]) as sst.py:83-99 yields them.  `consts` [Z * L, 4] and `zone_range` [Z, 2]
    (see build_zones) are on the device beside `frames`; with eval=True a batch carries, per row, the index into `consts` of its first
    target day and the position of its zone in `zone_range`."""

    step = 1
    var_names = list(VAR_NAMES)

    def __init__(self, data_dir, nt_cond, nt_pred, train, zones=range(1, 30), eval=False, device=None):
        device = require_gpu('SST', device)
        self.data_dir, self.zones, self.train, self.eval = data_dir, list(zones), train, eval
        self.nt_pred, self.zone_size = nt_pred, ZONE_SIZE
        frames, consts, zone_range, self.L = build_zones(data_dir, self.zones)
        first, self.len_ = item_table(len(self.zones), self.L, nt_cond, nt_pred, train)
        super().__init__(torch.from_numpy(frames).to(device), torch.from_numpy(first).to(device), nt_cond + nt_pred, nt_cond,
                         (1, ZONE_SIZE, ZONE_SIZE) if frames.shape[1] == ZONE_SIZE * ZONE_SIZE else (frames.shape[1],))
        self.consts = torch.from_numpy(consts).to(device)
        self.zone_range = torch.from_numpy(zone_range).to(device)

    def batch(self, item_idx, out_dtype=torch.float32):
        """As TimelineSet.batch; with eval=True also (day0 [B], zone [B]) int32 on the device."""
        item_idx, validate = self._device_index(item_idx)
        cond, target = self._gather(item_idx, validate, out_dtype)
        if not self.eval:
            return cond, target
        day0 = self.first[item_idx.long()] + self.nt_cond
        zone = torch.div(item_idx, self.len_, rounding_mode='floor').to(torch.int32)
        return cond, target, day0, zone

    def __getitem__(self, index):
        """(cond, target), and with eval=True the reference's seven values: the constants of the target days as [nt_pred, 1, 1] device
        tensors and the zone's name (sst.py:91-99)."""
        if not self.eval:
            return super().__getitem__(index)
        cond, target, day0, zone = self.batch([int(index)])
        d0 = int(day0[0])
        mu_norm, std_norm, mu_clim, std_clim = (self.consts[d0:d0 + self.nt_pred, k].reshape(-1, 1, 1) for k in range(4))
        return cond[0], target[0], mu_clim, std_clim, mu_norm, std_norm, self.zones[int(zone[0])]

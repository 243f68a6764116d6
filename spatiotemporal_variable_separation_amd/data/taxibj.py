"""TaxiBJ resident in HBM, batches gathered on the device (reference: var_sep/data/taxibj.py:16-268, itself taken from MIM).

The reference materialises every window on the host: `XC` is [N, len_closeness, 32, 32, 2] float64 -- 8x the data for the recipe's
4 + 4 frames -- and a DataLoader stacks the items.  Its windows are a SPARSE set (`STMatrix.create_dataset` drops every window that would
cross a missing half-hour, an incomplete day or a file boundary) and each is stored NEWEST FRAME FIRST (`depends = range(1,
len_closeness + 1)`: position k of an item is the frame k + 1 slots before its timestamp).  Here the normalised frames live in HBM once
as one fp32 [F, nb_flow * 32 * 32] tensor (the paper's set: ~184 MB), a window is an entry of an int32 table -- the index of the frame at
its position 0 -- and a batch is one gather launch read backwards (`vs_gather_timeline`, step -1) driven by the sampler's item indices.

Everything before the upload is `build_windows`, a pure NumPy function that needs no GPU, no pandas and no hard h5py dependency: file
reading, `remove_incomplete_days`, the clamp, the min-max fit on the train FRAMES and the window table follow the reference line by line,
so that items, their order and the train / test cut are the reference's, bit for bit.  One documented divergence: a year whose timestamps
are unsorted or duplicated raises ValueError (the reference would silently build items of non-contiguous frames).
"""
import datetime
import os

import numpy as np
import torch

from .device import TimelineSet, read_optional, require_gpu

YEARS = (13, 14, 15, 16)
H5_NAME = 'BJ{}_M32x32_T30_InOut.h5'
NPZ_NAME = 'BJ{}_M32x32_T30_InOut.npz'
CONVERSION_HINT = ("import h5py, numpy as np; f = h5py.File('{h5}', 'r')\n"
                   "np.savez('{npz}', data=f['data'][()], date=f['date'][()])")


class MinMaxNormalization:
    """Min-max scaling to [0, 1] with the surface of taxibj.py:139-165: `fit` records `_min` / `_max` of the array it is given (the train
    frames), `transform` and `inverse_transform` apply them.  Both are written as the reference evaluates them -- a leading `1. *`, the
    subtraction, ONE division by the range -- because the order of operations and NumPy's dtype promotion decide the last bit."""

    _min = None
    _max = None

    def fit(self, X):
        self._min, self._max = X.min(), X.max()

    def transform(self, X):
        return 1. * (X - self._min) / (self._max - self._min)

    def fit_transform(self, X):
        self.fit(X)
        return self.transform(X)

    def inverse_transform(self, X):
        return 1. * X * (self._max - self._min) + self._min


def _read_h5(h5py, path):
    f = h5py.File(path, 'r')
    data = f['data'][()]
    timestamps = f['date'][()]
    f.close()
    return data, timestamps


def load_stdata(data_dir, year):
    """(data [N, flows, 32, 32], timestamps [N] of bytes or str) of one year: the .h5 file through h5py when that module imports and the
    file exists (taxibj.py:103-108), else the .npz file with the same two arrays under the keys `data` and `date`."""
    data, timestamps = read_optional('h5py', os.path.join(data_dir, H5_NAME.format(year)), os.path.join(data_dir, NPZ_NAME.format(year)),
                                     _read_h5, lambda z: (z['data'], z['date']), 'year',
                                     CONVERSION_HINT.format(h5=H5_NAME.format(year), npz=NPZ_NAME.format(year)))
    data = np.asarray(data)
    timestamps = list(np.asarray(timestamps).tolist())
    if len(data) != len(timestamps):
        raise ValueError('%s: %d frames but %d timestamps' % (H5_NAME.format(year)[:-3], len(data), len(timestamps)))
    return data, timestamps


def timestamp_minutes(t, T=48):
    """Minutes since day 0 of the proleptic Gregorian calendar of a `YYYYMMDDSS` timestamp (bytes or str), in integers: the date and the
    hour / minute `string2timestamp` (taxibj.py:16-26) gives slot SS.  Consecutive slots are 24 * 60 // T minutes apart."""
    if isinstance(t, bytes):
        t = t.decode('ascii')
    year, month, day, slot = int(t[:4]), int(t[4:6]), int(t[6:8]), int(t[8:]) - 1
    time_per_slot = 24.0 / T
    num_per_T = T // 24
    hour, minute = int(slot * time_per_slot), (slot % num_per_T) * int(60.0 * time_per_slot)
    if not (0 <= hour < 24 and 0 <= minute < 60):        # datetime() of the reference raises the same error class
        raise ValueError('timestamp %r: slot %d is outside a day of %d slots' % (t, slot + 1, T))
    return (datetime.date(year, month, day).toordinal() * 24 + hour) * 60 + minute


def remove_incomplete_days(data, timestamps, T=48):
    """The filter of taxibj.py:184-207.  A day is kept when an entry of slot 1 is followed, exactly T - 1 entries later, by an entry of slot T
    (the scan then jumps past that day; any other entry advances it by one); every entry whose `YYYYMMDD` names a kept day survives, the
    rest -- days with a hole, a missing end or a late start -- go."""
    n, pos, kept_days = len(timestamps), 0, set()
    while pos < n:
        end = pos + T - 1
        if int(timestamps[pos][8:]) == 1 and end < n and int(timestamps[end][8:]) == T:
            kept_days.add(timestamps[pos][:8])
            pos += T
        else:
            pos += 1
    keep = [i for i, t in enumerate(timestamps) if t[:8] in kept_days]
    return data[keep], [timestamps[i] for i in keep]


def window_table(timestamps, len_closeness, T=48, what='the timeline'):
    """Indices i of `STMatrix.create_dataset` (taxibj.py:74-100): i >= len_closeness whose len_closeness preceding slots are all present.
    The frames are looked up through a slot -> index dictionary in which the last occurrence wins (`make_index`); every looked-up index
    must be i - j, else the timestamps are unsorted or duplicated and ValueError is raised."""
    minutes = [timestamp_minutes(t, T) for t in timestamps]
    offset = 24 * 60 // T
    get_index = {}
    for i, m in enumerate(minutes):
        get_index[m] = i
    out = []
    for i in range(len_closeness, len(minutes)):
        found = [get_index.get(minutes[i] - j * offset) for j in range(1, len_closeness + 1)]
        if any(f is None for f in found):
            continue
        if found != list(range(i - 1, i - 1 - len_closeness, -1)):
            raise ValueError('%s: the timestamps around %r are unsorted or duplicated (its %d preceding slots are at positions %s, not the %d '
                             'positions before it)' % (what, timestamps[i], len_closeness, found, len_closeness))
        out.append(i)
    return np.asarray(out, dtype=np.int64)


def build_windows(data_dir, T=48, nb_flow=2, len_closeness=None, len_test=48 * 7 * 4):
    """Host half of `TaxiBJ.make_datasets` (taxibj.py:217-259), NumPy only -> (frames, first, n_train, mmn):
      frames  fp32 [F, nb_flow * 32 * 32]: the kept frames of the four years in file order, min-max normalised with the reference's own
              expression in the dtype NumPy gives it, then rounded ONCE to fp32 (the `.float()` of `__getitem__`);
      first   int32 [N]: per window, the index of the frame at its position 0 (one slot before its timestamp); position k is frame
              first - k;
      n_train the windows [:n_train] are the train set, the rest the test set (`XC[:-len_test]` / `XC[-len_test:]`);
      mmn     the fitted MinMaxNormalization."""
    if len_closeness is None or int(len_closeness) < 1:
        raise ValueError('len_closeness (frames per item) must be a positive integer')
    len_closeness = int(len_closeness)
    data_all, timestamps_all = [], []
    for year in YEARS:
        data, timestamps = load_stdata(data_dir, year)
        data, timestamps = remove_incomplete_days(data, timestamps, T)
        data = data[:, :nb_flow]
        data[data < 0] = 0.
        data_all.append(data)
        timestamps_all.append(timestamps)

    data_train = np.vstack(data_all)[:-len_test]         # cuts FRAMES, not windows (taxibj.py:235)
    mmn = MinMaxNormalization()
    mmn.fit(data_train)
    del data_train
    frames = np.concatenate([np.asarray(mmn.transform(d)).astype(np.float32) for d in data_all], axis=0)
    frames = np.ascontiguousarray(frames.reshape(len(frames), -1))

    first, year_offset = [], 0
    for year, timestamps in zip(YEARS, timestamps_all):
        i = window_table(timestamps, len_closeness, T, what=H5_NAME.format(year)[:-3])
        first.append(year_offset + i - 1)
        year_offset += len(timestamps)
    first = np.concatenate(first)
    if year_offset >= 2 ** 31:
        raise ValueError('%d frames do not fit the int32 window table' % year_offset)
    n_windows = len(first)
    n_train = len(range(n_windows)[:-len_test])
    return frames, first.astype(np.int32), n_train, mmn


class TaxiBJ(TimelineSet):
    """One half (train or test) of the TaxiBJ windows: `frames` fp32 [F, elems] on the device (shared by both halves), `first` its own
    int32 window table on the device.  Items are (cond [nt_cond, flows, 32, 32], target [len_closeness - nt_cond, ...]), newest frame
    first, as taxibj.py:263-265 yields them."""

    step = -1

    def __init__(self, frames, first, nt_cond, len_closeness, mmn, frame_shape):
        super().__init__(frames, first, len_closeness, nt_cond, frame_shape)
        self.len_closeness, self.mmn = len_closeness, mmn

    @classmethod
    def make_datasets(cls, data_dir, T=48, nb_flow=2, len_closeness=None, len_test=48 * 7 * 4, nt_cond=4, device=None):
        """-> (train, test), as taxibj.py:217-261, on `device`."""
        device = require_gpu('TaxiBJ', device)
        frames, first, n_train, mmn = build_windows(data_dir, T, nb_flow, len_closeness, len_test)
        if not 0 <= nt_cond <= len_closeness:
            raise ValueError('nt_cond %d exceeds the %d frames of an item' % (nt_cond, len_closeness))
        shape = (nb_flow, 32, 32) if frames.shape[1] == nb_flow * 32 * 32 else (frames.shape[1],)
        frames = torch.from_numpy(frames).to(device)
        halves = [torch.from_numpy(np.ascontiguousarray(part)).to(device) for part in (first[:n_train], first[n_train:])]
        return tuple(cls(frames, part, nt_cond, int(len_closeness), mmn, shape) for part in halves)

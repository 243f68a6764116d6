"""Inputs of the TaxiBJ fixtures (tests/golden/taxibj), rebuilt from a seed by the fixture generator (tests/make_golden_taxibj.py) and by
the tests (tests/test_taxibj_cpu.py, tests/test_taxibj_gpu.py).  Nothing here imports the reference, and nothing of it is committed.

Four synthetic years (13..16) of DAYS days x 48 half-hour slots of [2, 32, 32] integer-valued float64 counts in [-3, 1300) (negatives
meet the clamp), arranged so that every filter of the loader has work:
  * year 13: one slot removed in the middle of day 3 -> an incomplete day, dropped whole, which leaves a gap in the timeline;
  * year 14: day 4 missing altogether -> a gap;
  * year 15: complete;
  * year 16: the last slot of the last day missing -> an incomplete last day.
That leaves 8 + 8 + 9 + 8 days = 1584 frames; with 8 frames per item 1536 windows (each of the 7 contiguous runs loses 8 -- and the
default test half of 1344 leaves 192 for training), with 5 frames per item 1549.  A few values of 2000 sit only inside the last 1344
frames, so the min-max fitted on the frames before them (`[:-len_test]` cuts frames, not windows) leaves test values above 1.
Timestamps are bytes for the years 13 and 14 and str for 15 and 16 in the .npz tree; the h5py stand-in delivers bytes, as h5py does.
"""
import datetime
import functools
import os

import numpy as np

from golden_util import install_standin, item_crcs, remove_standin  # noqa: F401  (item_crcs: used through this module)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'taxibj')

YEARS = (13, 14, 15, 16)
DAYS, T, SEED = 9, 48, 1316
START = {13: (2013, 7, 1), 14: (2014, 3, 1), 15: (2015, 2, 24), 16: (2015, 12, 27)}       # 15 crosses a month end, 16 a year end
BIG = 2000.0
H5_NAME = 'BJ{}_M32x32_T30_InOut.h5'
NPZ_NAME = 'BJ{}_M32x32_T30_InOut.npz'

# the two dataset calls of the fixture, and the evaluation run (the `vgg32_tiny` network of oracle/golden_configs.py: nt_cond 2)
CALLS = {'a': dict(len_closeness=8, len_test=1344, nt_cond=4), 'b': dict(len_closeness=5, len_test=60, nt_cond=2)}
WHOLE_ITEMS = [('a', 'train', 0), ('a', 'train', -1), ('a', 'test', 0), ('a', 'test', -1), ('b', 'train', 7), ('b', 'test', -1)]
PARAMS = dict(architecture='vgg', data='taxibj', nt_cond=2, nt_pred=2, offset=2, skipco=False)
N_TEST = 1344


@functools.lru_cache(maxsize=None)
def arrays():
    """{year: (data float64 [N, 2, 32, 32], date: list of N bytes `YYYYMMDDSS`)}."""
    rng = np.random.RandomState(SEED)
    out = {}
    for year in YEARS:
        day0 = datetime.date(*START[year])
        stamps = []
        for d in range(DAYS):
            day = day0 + datetime.timedelta(days=d)
            for s in range(1, T + 1):
                stamps.append((d, s, ('%04d%02d%02d%02d' % (day.year, day.month, day.day, s)).encode('ascii')))
        if year == 13:
            stamps = [q for q in stamps if (q[0], q[1]) != (3, 20)]
        elif year == 14:
            stamps = [q for q in stamps if q[0] != 4]
        elif year == 16:
            stamps = stamps[:-1]
        data = rng.randint(-3, 1300, size=(len(stamps), 2, 32, 32)).astype(np.float64)
        if year in (15, 16):                             # inside the last 1344 kept frames
            where = rng.randint(0, data.size, size=5)
            data.reshape(-1)[where] = BIG
        data.setflags(write=False)
        out[year] = (data, [q[2] for q in stamps])
    return out


def write_tree(data_dir):
    """The four `.npz` files (keys `data`, `date`) under `data_dir`."""
    os.makedirs(data_dir, exist_ok=True)
    for year, (data, date) in arrays().items():
        stamps = np.array(date) if year in (13, 14) else np.array([d.decode('ascii') for d in date])
        np.savez(os.path.join(data_dir, NPZ_NAME.format(year)), data=data, date=stamps)
    return data_dir


def touch_h5_tree(data_dir):
    """Empty `.h5` files: the loader opens a year through h5py only where its file exists; the stand-in below never reads them."""
    os.makedirs(data_dir, exist_ok=True)
    for year in YEARS:
        open(os.path.join(data_dir, H5_NAME.format(year)), 'wb').close()
    return data_dir


def install_fake_h5py(year_arrays=None):
    """Put a minimal stand-in `h5py` into sys.modules and return it: `File(name, mode)` with `__getitem__` ('data' / 'date' -> a fresh
    array, which `[()]` reads whole, timestamps as bytes), `close` and the context-manager protocol.  The year is read from the file's
    name; `year_arrays` defaults to arrays().  Undo with remove_fake_h5py()."""
    year_arrays = arrays() if year_arrays is None else year_arrays

    class File:
        def __init__(self, name, mode='r'):
            base = os.path.basename(str(name))
            self._data, self._date = year_arrays[int(base[2:4])]

        def __getitem__(self, key):
            return {'data': np.array(self._data), 'date': np.array(self._date, dtype='S10')}[key]

        def close(self):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            self.close()

    return install_standin('h5py', File=File)


def remove_fake_h5py():
    remove_standin('h5py')


def assemble(frames, first, items, len_closeness):
    """fp32 [n, len_closeness, 2, 32, 32] of the windows `items` from the host arrays of `build_windows`: position k is frame first - k."""
    rows = np.asarray(first)[np.asarray(items)].astype(np.int64)[:, None] - np.arange(len_closeness)[None]
    return np.asarray(frames)[rows].reshape(len(rows), len_closeness, 2, 32, 32)


def whole_item_key(call, half, index):
    return 'item_%s_%s_%s' % (call, half, str(index).replace('-', 'm'))

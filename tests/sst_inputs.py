"""Inputs of the SST fixtures (tests/golden/sst), rebuilt from a seed by the fixture generator (tests/make_golden_sst.py) and by the tests
(tests/test_sst_cpu.py, tests/test_sst_gpu.py).  Nothing here imports the reference, and nothing of it is committed.

Six synthetic zones (1, 2, 17..20) of L = 120 days of 64 x 64 fp32 `thetao`: a sum of a few drifting low-frequency sinusoids plus 0.1
noise, times a daily std in [0.6, 1.4], plus a daily mean in [0.5, 1.5].  `daily_mean` / `daily_std` are float32 for odd zones and float64
for even ones, so both of NumPy's promotions occur in the normalisation.  With L = 120 the test half starts at day 96; 2 + 10 days per item
leave 11 windows per zone (44 for the evaluation's zones 17-20), 2 + 2 days leave 91 per zone in the train half.
"""
import functools
import os

import numpy as np

from golden_util import install_standin, item_crcs, remove_standin  # noqa: F401  (item_crcs: used through this module)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'sst')

ZONES = (1, 2, 17, 18, 19, 20)
L, SIZE, SEED = 120, 64, 1720
NC_NAME = 'data_{}.nc'
NPZ_NAME = 'data_{}.npz'
VAR_NAMES = ('thetao', 'daily_mean', 'daily_std')

# the two dataset calls of the fixture, and the evaluation run (the `sst_skip` network of oracle/golden_configs.py: nt_cond 2, offset 0)
CALLS = {'test': dict(nt_cond=2, nt_pred=10, train=False, zones=(17, 18, 19, 20)), 'train': dict(nt_cond=2, nt_pred=2, train=True, zones=(2, 17, 1))}
WHOLE_ITEMS = [('test', -1), ('train', 100)]
PARAMS = dict(architecture='encoderSST', decoder_architecture='decoderSST', data='sst', nt_cond=2, nt_pred=2, offset=0, skipco=True)
EVAL_ZONES = (17, 18, 19, 20)
N_TEST = 44


@functools.lru_cache(maxsize=None)
def arrays():
    """{zone: {'thetao': fp32 [L, 64, 64], 'daily_mean': [L], 'daily_std': [L]}}."""
    out = {}
    y, x = np.meshgrid(np.arange(SIZE) / SIZE, np.arange(SIZE) / SIZE, indexing='ij')
    day = np.arange(L).reshape(L, 1, 1)
    for zone in ZONES:
        rng = np.random.RandomState(SEED + zone)
        field = np.zeros((L, SIZE, SIZE))
        for _ in range(4):
            fx, fy = rng.uniform(0.5, 2.0, size=2)
            amp, phase, drift = rng.uniform(0.4, 1.0), rng.uniform(0, 2 * np.pi), rng.uniform(-0.15, 0.15)
            field += amp * np.sin(2 * np.pi * (fx * x + fy * y)[None] + phase + drift * day)
        field += 0.1 * rng.standard_normal(field.shape)
        dtype = np.float32 if zone % 2 else np.float64
        daily_std = rng.uniform(0.6, 1.4, size=L).astype(dtype)
        daily_mean = rng.uniform(0.5, 1.5, size=L).astype(dtype)
        thetao = (field * daily_std.reshape(L, 1, 1) + daily_mean.reshape(L, 1, 1)).astype(np.float32)
        z = {'thetao': thetao, 'daily_mean': daily_mean, 'daily_std': daily_std}
        for a in z.values():
            a.setflags(write=False)
        out[zone] = z
    return out


def write_tree(data_dir, zones=ZONES, zone_arrays=None):
    """The `data_{zone}.npz` files (keys thetao, daily_mean, daily_std) under `data_dir`."""
    zone_arrays = arrays() if zone_arrays is None else zone_arrays
    os.makedirs(data_dir, exist_ok=True)
    for zone in zones:
        np.savez(os.path.join(data_dir, NPZ_NAME.format(zone)), **zone_arrays[zone])
    return data_dir


def touch_nc_tree(data_dir, zones=ZONES):
    """Empty `.nc` files: the loader opens a zone through netCDF4 only where its file exists; the stand-in below never reads them."""
    os.makedirs(data_dir, exist_ok=True)
    for zone in zones:
        open(os.path.join(data_dir, NC_NAME.format(zone)), 'wb').close()
    return data_dir


def install_fake_netcdf4(zone_arrays=None):
    """Put a minimal stand-in `netCDF4` into sys.modules and return it: `Dataset(fp, 'r').variables[name][:]` returns a fresh masked array
    (nothing masked), as netCDF4 does.  The zone is read from the file's name; `zone_arrays` defaults to arrays().  Undo with
    remove_fake_netcdf4()."""
    zone_arrays = arrays() if zone_arrays is None else zone_arrays

    class Variable:
        def __init__(self, a):
            self._a = a

        def __getitem__(self, key):
            return np.ma.masked_array(np.array(self._a)[key])

    class Dataset:
        def __init__(self, fp, mode='r'):
            base = os.path.basename(str(fp))
            zone = int(base[len('data_'):-len('.nc')])
            self.variables = {name: Variable(a) for name, a in zone_arrays[zone].items()}

        def close(self):
            pass

    return install_standin('netCDF4', Dataset=Dataset)


def remove_fake_netcdf4():
    remove_standin('netCDF4')


def assemble(frames, first, items, seq_len):
    """fp32 [n, seq_len, 1, 64, 64] of the windows `items` from the host arrays: position k is day first + k."""
    rows = np.asarray(first)[np.asarray(items)].astype(np.int64)[:, None] + np.arange(seq_len)[None]
    return np.asarray(frames)[rows].reshape(len(rows), seq_len, 1, SIZE, SIZE)


def whole_item_key(call, index):
    return 'item_%s_%s' % (call, str(index).replace('-', 'm'))


def _band(n, sigma, like):
    """[n, n - 10] fp64: column j holds the normalised 11-tap Gaussian at rows j .. j + 10 (the 2-D window of the SSIM is the outer product
    of two of these: softmax of a sum = product of softmaxes)."""
    import torch
    x = torch.arange(11, dtype=torch.float64) - 5.0
    g = torch.exp(-x * x / (2.0 * sigma * sigma))
    g = g / g.sum()
    m = torch.zeros((n, n - 10), dtype=torch.float64)
    for j in range(n - 10):
        m[j:j + 11, j] = g
    return m.to(like.device)


def metrics_fp64(pred, target, consts, lo, hi, k1=0.01, k2=0.03, sigma=1.5):
    """fp64 statement of test/sst/test.py:57-71 on torch tensors (any device): pred, target [N, T, H, W]; consts [N, T, 4] = (mu_norm,
    std_norm, mu_clim, std_clim) of the T target days of each window; lo, hi [N] -> (mse [N, T], ssim [N, T, T]) in fp64.  Frame t is paired
    with the constants of every day c; the Gaussian filter is two fp64 matrix products per map."""
    import torch
    pred, target, consts, lo, hi = (torch.as_tensor(a).double() for a in (pred, target, consts, lo, hi))
    N, T, H, W = pred.shape
    mn, sn, mc, sc = (consts[:, None, :, k, None, None] for k in range(4))            # [N, 1, T, 1, 1]
    p = (pred[:, :, None] * sn + mn) * sc + mc                                          # [N, T, T, H, W]
    t = (target[:, :, None] * sn + mn) * sc + mc
    mse = (p - t).pow(2).mean(dim=(2, 3, 4))
    lo, hi = lo.view(N, 1, 1, 1, 1), hi.view(N, 1, 1, 1, 1)
    p, t = (p - lo) / (hi - lo), (t - lo) / (hi - lo)
    gh, gw = _band(H, sigma, p).t(), _band(W, sigma, p)

    def filt(a):
        return gh @ a @ gw

    c1, c2 = k1 ** 2, k2 ** 2
    mu1, mu2 = filt(p), filt(t)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = filt(p * p) - mu1_sq, filt(t * t) - mu2_sq, filt(p * t) - mu12
    ssim = ((2 * mu12 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))
    return mse, ssim.mean(dim=(3, 4))

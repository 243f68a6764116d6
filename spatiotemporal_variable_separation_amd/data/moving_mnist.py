"""Moving MNIST generated on the device (reference: data/moving_mnist.py:39-341).

Same class name, constructor / `make_dataset` arguments and sampling semantics as the reference: every training item is a fresh
video of `num_digits` digits bouncing elastically inside a `nx` x `nx` frame, built from five draws of the GLOBAL NumPy stream
per digit (digit index, start row, start column, row speed, column speed -- `moving_mnist.py:121-123, 156-160`).  What differs is
where the work happens: the host only draws those integers (in the reference's order, so a seeded single-process run yields the
reference's videos bit for bit) and ONE kernel launch (`vs_moving_mnist_batch`) computes the trajectories and renders the whole
batch into HBM.  A 4-worker host generator tops out far below the > 100 k frames/s the MI355X training step consumes.

Digits come from the raw MNIST idx files under `data_dir` (the files torchvision downloads: `MNIST/raw/train-images-idx3-ubyte[.gz]`;
torchvision itself is not needed), or -- `data_dir='synthetic_digits'` -- from seeded 28x28 blobs for benchmarks and tests.
Both variants are generated on the device.  The deterministic one (the one main.py constructs by default) as above.  The stochastic one
(`deterministic=False`, `main --mnist_stochastic`) redraws the speed vector from the stream at every bounce (`moving_mnist.py:232-234`), so
the outputs a trajectory takes depend on the trajectory: with a `DeviceRandomState` ONE launch (`vs_mmnist_stochastic_trajectories`) draws and
walks the whole batch from the stream in HBM and `vs_moving_mnist_place` renders it; otherwise `draw_stochastic` makes the same draws from
the host stream in a Python loop.  The stochastic TEST set (`smmnist_test_*.npz`, `stochastic_test_set`) is two launches: the same walk
kernel over all its trajectories, from the stream as the permutation of the test images leaves it, and `vs_moving_mnist_testset_place`.
"""
import gzip
import os

import numpy as np
import torch

from .numpy_stream import DeviceRandomState


def synthetic_digits(n=256, size=28, seed=1234):
    """Seeded digit-like blobs (uint8 [n, size, size]): a few soft strokes on a dark background, MNIST's value range."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float32)
    out = np.zeros((n, size, size), dtype=np.float32)
    for i in range(n):
        img = np.zeros((size, size), dtype=np.float32)
        for _ in range(rng.randint(2, 5)):
            cy, cx = rng.uniform(6, size - 6, 2)
            ang, length, width = rng.uniform(0, np.pi), rng.uniform(4, 10), rng.uniform(1.0, 2.2)
            dy, dx = np.sin(ang), np.cos(ang)
            along = (yy - cy) * dy + (xx - cx) * dx
            across = -(yy - cy) * dx + (xx - cx) * dy
            img += np.exp(-(across / width) ** 2) * (np.abs(along) <= length)
        out[i] = np.clip(img, 0, 1) * 255.0
    return out.astype(np.uint8)


def read_mnist_images(data_dir, train=True):
    """uint8 [N, 28, 28] from the idx3-ubyte file torchvision's MNIST keeps under <data_dir>/MNIST/raw (gzip or plain)."""
    stem = 'train-images-idx3-ubyte' if train else 't10k-images-idx3-ubyte'
    for base in (os.path.join(data_dir, 'MNIST', 'raw'), data_dir):
        for name, opener in ((stem, open), (stem + '.gz', gzip.open)):
            path = os.path.join(base, name)
            if os.path.exists(path):
                with opener(path, 'rb') as f:
                    raw = f.read()
                magic, n, h, w = np.frombuffer(raw[:16], dtype='>i4')
                if magic != 2051:
                    raise ValueError('%s is not an idx3-ubyte image file' % path)
                return np.frombuffer(raw, dtype=np.uint8, offset=16).reshape(int(n), int(h), int(w)).copy()
    raise FileNotFoundError('no %s[.gz] under %s (expected the raw MNIST files; pass data_dir=synthetic_digits for seeded blobs)'
                            % (stem, data_dir))


def read_mnist_labels(data_dir, train=False):
    """uint8 [N] from the idx1-ubyte label file beside the images (`read_mnist_images` lists the locations; gzip or plain)."""
    stem = 'train-labels-idx1-ubyte' if train else 't10k-labels-idx1-ubyte'
    for base in (os.path.join(data_dir, 'MNIST', 'raw'), data_dir):
        for name, opener in ((stem, open), (stem + '.gz', gzip.open)):
            path = os.path.join(base, name)
            if os.path.exists(path):
                with opener(path, 'rb') as f:
                    raw = f.read()
                magic, n = np.frombuffer(raw[:8], dtype='>i4')
                if magic != 2049:
                    raise ValueError('%s is not an idx1-ubyte label file' % path)
                return np.frombuffer(raw, dtype=np.uint8, offset=8)[:int(n)].copy()
    raise FileNotFoundError('no %s[.gz] under %s (expected the raw MNIST files)' % (stem, data_dir))


def draw_test_set(n_images, digit_shape, frame_size, max_speed, num_digits, seed):
    """The draws of the reference's preprocessing/mnist/make_test_set.py, in its order, from the GLOBAL NumPy stream (which it reseeds):
    np.random.seed(seed), the permutation of the test images, then per video and digit the four randint calls of `_compute_trajectory`
    (start row, start column, row speed, column speed).  -> (digits_idx int64 [n_images], init int32 [n_images // num_digits, num_digits,
    5]) with init[v, n, 0] = digits_idx[v * num_digits + n]; the n_images % num_digits last images of the permutation are unused."""
    h, w = digit_shape
    np.random.seed(seed)
    digits_idx = np.random.permutation(n_images)
    n_videos = n_images // num_digits
    init = np.empty((n_videos, num_digits, 5), dtype=np.int32)
    rnd = np.random.randint
    for v in range(n_videos):
        for n in range(num_digits):
            init[v, n] = (digits_idx[v * num_digits + n], rnd(0, frame_size - h + 1), rnd(0, frame_size - w + 1),
                          rnd(-max_speed, max_speed + 1), rnd(-max_speed, max_speed + 1))
    return digits_idx, init


def stochastic_test_set(test_images, frame_size, max_speed, num_digits, seed, seq_len, fp32=False, time_major=True):
    """The STOCHASTIC test set (`smmnist_test_*.npz`): the reference's preprocessing/mnist/make_test_set.py loop with a sampler built with
    deterministic=False, which redraws the speed vector from the global stream at every bounce.  test_images: uint8 [n_images, h, w] on the
    device.  The host only seeds the global NumPy stream and draws the permutation of the images, as the reference does; the stream's state
    then goes to HBM, ONE launch draws and walks all n_videos * num_digits trajectories in the stream's order (four prefix draws each: start
    row, start column, row speed, column speed -- ops.mmnist_stochastic_trajectories) and ONE launch renders the frames from the positions
    (ops.moving_mnist_testset_place).  -> (digits_idx int64 [n_images], frames, latents int32 [seq_len, n_videos, num_digits, 4]); frames
    as ops.moving_mnist_testset gives them for the same `fp32` / `time_major`.  Both launches are validated (two host syncs: the set is made
    once), and the global stream is left where the reference's script leaves it: past the last draw of the last trajectory."""
    from .. import ops
    n_images, h, w = (int(v) for v in test_images.shape)
    x_max, y_max, s = frame_size - h, frame_size - w, max_speed
    if min(x_max, y_max) < 1:
        raise ValueError('stochastic Moving MNIST: a %d x %d digit fills the %d x %d frame along an axis (unsupported)'
                         % (h, w, frame_size, frame_size))
    np.random.seed(seed)
    digits_idx = np.random.permutation(n_images)
    n_videos = n_images // num_digits
    rs = DeviceRandomState(None, test_images.device)
    _, positions, latents, _ = ops.mmnist_stochastic_trajectories(rs.state, n_videos * num_digits, seq_len, (0, 0, -s, -s),
                                                                  (x_max + 1, y_max + 1, s + 1, s + 1), x_max, y_max, s, latents=True)
    used = torch.from_numpy(digits_idx[:n_videos * num_digits].astype(np.int32)).to(test_images.device).view(n_videos, num_digits)
    frames = ops.moving_mnist_testset_place(test_images, positions.view(seq_len, n_videos, num_digits, 2), used, frame_size, fp32=fp32,
                                            time_major=time_major)
    np.random.set_state(rs.get_state())
    return digits_idx, frames, latents.view(seq_len, n_videos, num_digits, 4)


_EPS = 1e-8


def _stochastic_collision(rnd, sx, sy, dx, dy, x_max, y_max, max_speed):
    """`_process_collision` of the reference with deterministic=False (moving_mnist.py:172-253) in Python floats: while the digit is outside
    [0, x_max] x [0, y_max], find where it left, redraw the speed vector, mirror it off the edges that were hit and spend the rest of the step."""
    left, upper, right, bottom = sx < -_EPS, sy < -_EPS, sx > x_max + _EPS, sy > y_max + _EPS
    cx = cy = 0
    while left or right or upper or bottom:
        if dx == 0:
            cx, cy = sx, (0 if upper else y_max)
        elif dy == 0:
            cx, cy = (0 if left else x_max), sy
        else:
            a = dy / dx
            b = sy - a * sx
            for edge, lim in ((0, 0), (1, x_max)):                    # left, right: where the line meets the row lim
                if (left, right)[edge]:
                    y = a * lim + b
                    hit = -_EPS <= y <= y_max + _EPS
                    left, right = (hit, right) if edge == 0 else (left, hit)
                    if hit:
                        cx, cy = lim, y
            for edge, lim in ((0, 0), (1, y_max)):                    # upper, bottom: where it meets the column lim
                if (upper, bottom)[edge]:
                    x = (lim - b) / a
                    hit = -_EPS <= x <= x_max + _EPS
                    upper, bottom = (hit, bottom) if edge == 0 else (upper, hit)
                    if hit:
                        cx, cy = x, lim
        p = (sx - cx) / dx if dx != 0 else (sy - cy) / dy
        dx, dy = rnd(-max_speed, max_speed + 1), rnd(-max_speed, max_speed + 1)     # dx first
        dx = abs(dx) if left else -abs(dx) if right else dx
        dy = abs(dy) if upper else -abs(dy) if bottom else dy
        sx, sy = cx + dx * p, cy + dy * p
        left, upper, right, bottom = sx < -_EPS, sy < -_EPS, sx > x_max + _EPS, sy > y_max + _EPS
    return sx, sy, dx, dy


_GENERATED = {}                  # the test sets generated in this process: one per (files, geometry, seed, device, variant)


def forget_generated():
    """Release the test sets that `MovingMNIST.generated` keeps for the life of the process (8.2 GB of HBM for the reference's set); the
    next call generates again.  Also the way to pick up idx files that changed under the same path: the key is the path, not the contents."""
    _GENERATED.clear()


class MovingMNIST:
    """Device-resident Moving MNIST.  `train=True`: videos generated per batch (`batch(B)` / DeviceMovingLoader); `train=False`: the
    precomputed test videos of the reference (`[s]mmnist_test_<n>digits_<nx>.npz`) kept in HBM."""
    eps = 1e-8
    device_resident = True
    generated_on_device = True
    rng = None                   # None: the global NumPy stream (the reference's); a np.random.RandomState: a private stream on the host;
                                 # a DeviceRandomState (data/numpy_stream.py): a private stream in HBM, drawn from by one launch per batch

    def __init__(self, data, nx, nt_cond, seq_len, max_speed, deterministic, num_digits, train, device='cuda'):
        self.frame_size, self.nt_cond, self.seq_len = nx, nt_cond, seq_len
        self.max_speed, self.deterministic, self.num_digits, self.train = max_speed, deterministic, num_digits, train
        self.device = torch.device(device)
        if train:
            arr = np.ascontiguousarray(np.stack([np.asarray(d, dtype=np.uint8) for d in data]) if not isinstance(data, np.ndarray) else data)
            assert arr.dtype == np.uint8 and arr.ndim == 3, 'digits: uint8 [N, h, w]'
            self.digit_shape = (int(arr.shape[1]), int(arr.shape[2]))
            self.n_source = int(arr.shape[0])
            self.data = torch.from_numpy(arr).to(self.device)
            if not deterministic and min(nx - self.digit_shape[0], nx - self.digit_shape[1]) < 1:
                raise ValueError('stochastic Moving MNIST: a %d x %d digit fills the %d x %d frame along an axis (unsupported)'
                                 % (self.digit_shape + (nx, nx)))
        elif isinstance(data, torch.Tensor):                     # `generated`: fp32 [N, T, 1, nx, nx], already in HBM
            self.data = data
        else:
            self.data = torch.stack([torch.as_tensor(np.asarray(v), dtype=torch.float32) for v in data]).to(self.device)

    def __len__(self):
        return 200000 if self.train else int(self.data.shape[0])       # moving_mnist.py:104-111: arbitrary epoch length when training

    def draw(self, batch):
        """The reference's draws for `batch` consecutive items from the global NumPy stream (moving_mnist.py:121-123, 156-160): int32
        [batch, num_digits, 5], a host array -- or, when `rng` is a DeviceRandomState, a device tensor with the same values from ONE launch
        (ops.mt19937_randint) and no upload or synchronisation."""
        h, w = self.digit_shape
        if isinstance(self.rng, DeviceRandomState):
            lows = (0, 0, 0, -self.max_speed, -self.max_speed)
            highs = (self.n_source, self.frame_size - h + 1, self.frame_size - w + 1, self.max_speed + 1, self.max_speed + 1)
            return self.rng.randint_table(lows, highs, batch * self.num_digits).view(batch, self.num_digits, 5)
        rnd = (self.rng or np.random).randint
        init = np.empty((batch, self.num_digits, 5), dtype=np.int32)
        for b in range(batch):
            for n in range(self.num_digits):
                init[b, n, 0] = rnd(self.n_source)
                init[b, n, 1] = rnd(0, self.frame_size - h + 1)
                init[b, n, 2] = rnd(0, self.frame_size - w + 1)
                init[b, n, 3] = rnd(-self.max_speed, self.max_speed + 1)
                init[b, n, 4] = rnd(-self.max_speed, self.max_speed + 1)
        return init

    def render(self, init, out_dtype=torch.float32):
        """init int32 [B, num_digits, 5] (host array or device tensor) -> videos [B, seq_len, 1, nx, nx] on the device."""
        if not isinstance(init, torch.Tensor):
            init = torch.from_numpy(np.ascontiguousarray(init, dtype=np.int32)).to(self.device, non_blocking=True)
        from .. import ops
        return ops.moving_mnist_batch(self.data, init, self.seq_len, self.frame_size, out_dtype)

    def draw_stochastic(self, batch):
        """The stochastic variant's draws AND walks for `batch` consecutive items (moving_mnist.py:119-123, 153-170, 230-234): (desc int32
        [batch, 1 + num_digits] = (item, its digits' indices), positions int32 [seq_len, batch, num_digits, 2] = (row, column) per frame),
        the operands of ops.moving_mnist_place.  When `rng` is a DeviceRandomState both are device tensors from ONE launch
        (ops.mmnist_stochastic_trajectories) with no upload or synchronisation; otherwise host arrays from a Python loop over the host
        stream, the same draws in the same order."""
        h, w = self.digit_shape
        x_max, y_max, s, nd = self.frame_size - h, self.frame_size - w, self.max_speed, self.num_digits
        if isinstance(self.rng, DeviceRandomState):
            _, positions, _, desc = self.rng.stochastic_trajectories(batch * nd, self.seq_len, (0, 0, 0, -s, -s),
                                                                     (self.n_source, x_max + 1, y_max + 1, s + 1, s + 1), x_max, y_max, s, desc_nd=nd)
            return desc, positions.view(self.seq_len, batch, nd, 2)
        rnd = (self.rng or np.random).randint
        desc = np.empty((batch, 1 + nd), dtype=np.int32)
        positions = np.empty((self.seq_len, batch, nd, 2), dtype=np.int32)
        for b in range(batch):
            desc[b, 0] = b
            for n in range(nd):
                desc[b, 1 + n] = rnd(self.n_source)
                sx, sy = rnd(0, x_max + 1), rnd(0, y_max + 1)
                dx, dy = rnd(-s, s + 1), rnd(-s, s + 1)
                for t in range(self.seq_len):
                    sx, sy, dx, dy = _stochastic_collision(rnd, sx, sy, dx, dy, x_max, y_max, s)
                    positions[t, b, n] = (int(round(sx)), int(round(sy)))
                    sy += dy
                    sx += dx
        return desc, positions

    def render_stochastic(self, desc, positions, out_dtype=torch.float32):
        """(desc, positions) of `draw_stochastic` (host arrays or device tensors) -> videos [B, seq_len, 1, nx, nx] on the device: the digits
        summed at their positions, min(., 255), / 255 (ops.moving_mnist_place, the arithmetic of the deterministic renderer)."""
        from .. import ops
        if not isinstance(desc, torch.Tensor):
            desc = torch.from_numpy(desc).to(self.device, non_blocking=True)
            positions = torch.from_numpy(positions).to(self.device, non_blocking=True)
        return ops.moving_mnist_place(self.data, positions, desc, self.seq_len, self.frame_size, out_dtype, validate=False)

    def batch(self, batch, out_dtype=torch.float32):
        """(cond, target) of `batch` fresh videos (training) -- `__getitem__` of the reference for a whole batch."""
        if self.deterministic:
            x = self.render(self.draw(batch), out_dtype)
        else:
            x = self.render_stochastic(*self.draw_stochastic(batch), out_dtype)
        return x[:, :self.nt_cond], x[:, self.nt_cond:]

    def __getitem__(self, index):
        if not self.train:
            v = self.data[index]
            return v[:self.nt_cond] / 255, v[self.nt_cond:self.seq_len] / 255
        cond, target = self.batch(1)
        return cond[0], target[0]

    @classmethod
    def make_dataset(cls, data_dir, nx, nt_cond, seq_len, max_speed, deterministic, num_digits, train, device='cuda', seed=None, load=None, report=None,
                     foreign=None, finder=None):
        """load: who decompresses the test-set file (utils/loadz.npz_loader: the keyword, then VARSEP_NPZ_LOAD, then 'host').  'host' is
        np.load and the host conversion, as before; 'device' inflates `sequences` in HBM (utils/loadz.load), where it stays uint8 until the
        [T, N, ...] -> fp32 [N, T, ...] step, also done there.  `.data` is the same bit for bit.  report: optional dict for
        utils/loadz.load's record of the route `sequences` took.  foreign: with 'device', who decompresses a file that is not cut at sync
        markers, as np.savez_compressed writes it (utils/loadz.npz_foreign: the keyword, then VARSEP_NPZ_FOREIGN, then 'host'), read here
        with the first rule and handed on when it is not the default.  finder: with both 'device', which block headers are found
        (utils/loadz.npz_finder: the keyword, then VARSEP_NPZ_FINDER, then 'dynamic'), read and handed on in the same way."""
        if train:
            data = synthetic_digits(seed=seed or 1234) if data_dir == 'synthetic_digits' else read_mnist_images(data_dir, train=True)
        else:
            from ..utils import loadz
            prefix = '' if deterministic else 's'
            path = os.path.join(data_dir, f'{prefix}mmnist_test_{num_digits}digits_{nx}.npz')
            how, who, which = loadz.npz_loader(load), loadz.npz_foreign(foreign), loadz.npz_finder(finder)
            if how == 'device':
                extra = {} if foreign is None and who == 'host' else {'foreign': who}
                if finder is not None or which != 'dynamic':
                    extra['finder'] = which
                sequences = loadz.load(path, device, keys=('sequences',), load='device', report=report, **extra)['sequences']
                if sequences.dtype == torch.uint8:
                    from .. import ops
                    data = ops.u8_tn_to_f32_nt(sequences)
                else:                                                       # (a file of another dtype: `astype(np.single)` as the host does it)
                    data = sequences.transpose(0, 1).to(torch.float32).contiguous()
            else:
                dataset = np.load(path, allow_pickle=True)
                sequences = dataset['sequences']
                data = [sequences[:, i].astype(np.single) for i in range(sequences.shape[1])]
        return cls(data, nx, nt_cond, seq_len, max_speed, deterministic, num_digits, train, device=device)

    @staticmethod
    def generated_key(data_dir, nx, max_speed, num_digits, device, seed=42, file_seq_len=100, deterministic=True):
        """What identifies a set kept by `generated`: the files' path, the geometry, the seed, the device and the variant."""
        key = (os.path.abspath(data_dir), nx, max_speed, num_digits, seed, file_seq_len, str(torch.device(device)))
        return key if deterministic else key + ('stochastic',)

    @classmethod
    def generated(cls, data_dir, nx, nt_cond, seq_len, max_speed, num_digits, device, seed=42, file_seq_len=100, deterministic=True):
        """The `train=False` set without its file: the videos `preprocessing/mnist/make_test_set.py --seed seed --seq_len file_seq_len`
        would write from the t10k idx files under `data_dir`, rendered straight into HBM by one fp32 launch (vs_moving_mnist_testset).
        `.data` equals, bit for bit, what `make_dataset(train=False)` loads from that file.  deterministic=False: the stochastic set that
        `make_test_set.py --stochastic` writes (`stochastic_test_set`: one walk launch and one fp32 render launch), which equals what
        `make_dataset(train=False, deterministic=False)` loads; the two variants are kept apart.  The object also keeps `latents` (int32
        [file_seq_len, N, num_digits, 4] on the device), `test_images` (the t10k images, uint8 on the device, file order) and `digits_idx`
        (the permutation: video v shows images digits_idx[v * num_digits + n]).  The global NumPy stream is left as it was found, and a
        set is generated once per process: a second call with the same path, geometry, seed and device SHARES the tensors, so `.data`,
        `latents` and `test_images` are read-only to every holder (`forget_generated()` releases them)."""
        from .. import ops
        device = torch.device(device)
        key = cls.generated_key(data_dir, nx, max_speed, num_digits, device, seed, file_seq_len, deterministic)
        if key not in _GENERATED:
            images = read_mnist_images(data_dir, train=False)
            test_images = torch.from_numpy(images).to(device)
            state = np.random.get_state()
            try:
                if deterministic:
                    digits_idx, init = draw_test_set(len(images), images.shape[1:], nx, max_speed, num_digits, seed)
                    frames, latents = ops.moving_mnist_testset(test_images, init, file_seq_len, nx, fp32=True, time_major=False)
                else:
                    digits_idx, frames, latents = stochastic_test_set(test_images, nx, max_speed, num_digits, seed, file_seq_len, fp32=True,
                                                                      time_major=False)
            finally:
                np.random.set_state(state)
            _GENERATED[key] = (frames, latents, test_images, digits_idx)
        frames, latents, test_images, digits_idx = _GENERATED[key]
        ds = cls(frames, nx, nt_cond, seq_len, max_speed, bool(deterministic), num_digits, False, device=device)
        ds.latents, ds.test_images, ds.digits_idx = latents, test_images, digits_idx
        return ds


class DeviceMovingLoader:
    """`DataLoader(MovingMNIST, batch_size, shuffle=True)` of main.py:113 for the device generator: len(dataset) // batch_size
    (+1 ragged) batches per epoch, each rendered by one launch.  Item indices are irrelevant to a generator, so no sampler runs."""

    def __init__(self, dataset, batch_size, drop_last=False, out_dtype=torch.float32, world=1, epoch_len=None):
        self.dataset, self.batch_size, self.drop_last, self.out_dtype = dataset, batch_size, drop_last, out_dtype
        self.sampler = None
        self.n_items = (epoch_len if epoch_len is not None else len(dataset)) // max(world, 1)

    def __len__(self):
        n = self.n_items
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        n = self.n_items
        for start in range(0, n, self.batch_size):
            size = min(self.batch_size, n - start)
            if size < self.batch_size and self.drop_last:
                return
            yield self.dataset.batch(size, self.out_dtype)

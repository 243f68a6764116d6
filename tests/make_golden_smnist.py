"""Generate tests/golden/smnist.npz by running the REFERENCE's own stochastic Moving-MNIST sampler (`var_sep.data.moving_mnist.MovingMNIST`
with deterministic=False: `_compute_trajectory`, `_process_collision`, the intersections, `__getitem__`), imported read-only, on the cases
of tests/smnist_inputs.py.

TEST INFRASTRUCTURE ONLY; runs where the reference is:   python tests/make_golden_smnist.py

The reference module does `from torchvision import datasets` at import time; torchvision is only used by `make_dataset(train=True)` to READ
the MNIST files, which this script never calls, so an empty placeholder module satisfies that line (as in oracle/make_golden_mmnist.py).
The restatement tests/smnist_ref.py must reproduce every value -- prefix draws, trajectories, final stream state, frames -- before the file
is written.  The file holds data only: per case the start state, the geometry, the calls, `pre`, the trajectories [n, T, 4] and the final
state; and the frames of `__getitem__` for 3 items x 2 digits x 6 frames of the blobs at frame sizes 64 and 32."""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
REF = os.environ.get('VARSEP_REFERENCE', '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import smnist_inputs as SI      # noqa: E402
import smnist_ref               # noqa: E402
from oracle import mmnist_ref   # noqa: E402


def reference_class():
    if 'torchvision' not in sys.modules:             # see the module docstring
        tv = types.ModuleType('torchvision')
        tv.datasets = types.ModuleType('torchvision.datasets')
        sys.modules['torchvision'], sys.modules['torchvision.datasets'] = tv, tv.datasets
    sys.path.insert(0, REF)
    from var_sep.data.moving_mnist import MovingMNIST
    return MovingMNIST


def reference_sampler(MovingMNIST):
    """The reference's own calls on the GLOBAL stream, which is set from and copied back to `rs` round every call."""
    def make(rs, watch):
        def sampler(c, n, cols, x_max, y_max, start):
            ds = MovingMNIST([None] * c['n_source'], c['frame'], 1, c['seq_len'], c['max_speed'], False, 1, True)
            np.random.set_state(rs.get_state())
            pre, traj = [], []
            for i in range(n):
                if c['n_pre'] == 5:
                    idx = np.random.randint(len(ds.data))                        # moving_mnist.py:120
                    t = ds._compute_trajectory(*c['digit'])
                    pre.append([idx] + list(t[0][:2]) + [None, None])            # the start speed is not returned: taken from the restatement below
                elif c['n_pre'] == 4:
                    t = ds._compute_trajectory(*c['digit'])
                    pre.append(list(t[0][:2]) + [None, None])
                else:
                    t = ds._compute_trajectory(*c['digit'], init_cond=tuple(int(v) for v in start[i]))
                    pre.append([])
                traj.append(t)
            rs.set_state(np.random.get_state())
            return pre, traj
        return sampler
    return make


def main():
    MovingMNIST = reference_class()
    kept = np.random.get_state()
    out = {}
    mine = SI.numpy_results()
    for c in SI.cases():
        name = c['name']
        cols, x_max, y_max = SI.geometry(c)
        rs = SI.random_state_at(c['state'])
        sampler = reference_sampler(MovingMNIST)(rs, None)
        pres, trajs = [], []
        for k, n in enumerate(c['calls']):
            pre, traj = sampler(c, n, cols, x_max, y_max, c['starts'][k] if c['starts'] else None)
            my_pre, my_traj = mine[name][0][k]
            traj = np.asarray(traj, dtype=np.int32).reshape(n, c['seq_len'], 4)
            assert np.array_equal(traj, my_traj), 'tests/smnist_ref.py differs from the reference (trajectories): ' + name
            # the prefix: what the reference returns of it (digit index, start position: no bounce at t = 0) must be the restatement's; the
            # start speed is consumed inside _compute_trajectory and shows in the trajectory, which is equal
            for got, want in zip(pre, my_pre):
                assert all(g is None or int(g) == int(w) for g, w in zip(got, want)) and len(got) == len(want), name
            pres.append(my_pre)
            trajs.append(traj)
        final = SI.state_words(rs)
        assert np.array_equal(final, mine[name][1]), 'tests/smnist_ref.py differs from the reference (stream state): ' + name
        out[name + ':state'] = np.asarray(c['state'])
        out[name + ':geom'] = np.array([c['frame'], c['digit'][0], c['digit'][1], c['max_speed'], c['seq_len'], c['n_source'], c['n_pre']], dtype=np.int64)
        out[name + ':calls'] = np.array(c['calls'], dtype=np.int64)
        out[name + ':pre'] = np.concatenate(pres).astype(np.int32).reshape(sum(c['calls']), c['n_pre'])
        out[name + ':traj'] = np.concatenate(trajs).astype(np.int32).reshape(sum(c['calls']), c['seq_len'], 4)
        out[name + ':final'] = final
        if c['starts']:
            out[name + ':start'] = np.concatenate(c['starts'])
        print('%-28s %4d trajectories of %3d frames; restatement identical' % (name, sum(c['calls']), c['seq_len']))
    digits = mmnist_ref.blobs()
    for key, frame, seed in SI.FRAME_SETS:
        ds = MovingMNIST([d for d in digits], frame, SI.FRAME_COND, SI.FRAME_LEN, 4, False, SI.FRAME_DIGITS, True)
        np.random.seed(seed)
        start = SI.state_words(np.random)
        vids = []
        for i in range(SI.FRAME_ITEMS):
            cond, target = ds[i]
            vids.append(np.concatenate([cond.numpy(), target.numpy()], axis=0))
        ref = np.stack(vids)
        final = SI.state_words(np.random)
        rs = SI.random_state_at(start)                                          # the restatement: same draws, same compositing
        x = np.zeros_like(ref)
        room = frame - 28
        for i in range(SI.FRAME_ITEMS):
            pre, traj = smnist_ref.sample(rs.randint, SI.FRAME_DIGITS, SI.FRAME_LEN, [(0, len(digits)), (0, room + 1), (0, room + 1), (-4, 5), (-4, 5)],
                                          room, room, 4)
            for q, tr in zip(pre, traj):
                for t, (px, py, _, _) in enumerate(tr):
                    x[i, t, 0, px:px + 28, py:py + 28] += digits[q[0]]
        x[x > 255] = 255
        x = x / 255
        assert x.dtype == ref.dtype == np.float32 and np.array_equal(x, ref), 'tests/smnist_ref.py differs from the reference (frames): ' + key
        assert np.array_equal(SI.state_words(rs), final), key
        u8 = np.round(ref * 255).astype(np.uint8)                                # exact: frames are k / 255 with integer k <= 255
        assert np.array_equal(u8.astype(np.float32) / 255, ref)
        out[key + ':state'], out[key + ':final'], out[key + ':u8'] = start, final, u8
        print('%-28s %d items, %d non-zero pixels; restatement identical' % (key, SI.FRAME_ITEMS, int((ref > 0).sum())))
    np.random.set_state(kept)
    np.savez_compressed(SI.GOLDEN, **out)
    print('wrote %s (%.1f KB)' % (SI.GOLDEN, os.path.getsize(SI.GOLDEN) / 1e3))


if __name__ == '__main__':
    main()

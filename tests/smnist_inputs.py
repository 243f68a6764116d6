"""Cases of the stochastic Moving-MNIST trajectory tests (tests/test_smnist_cpu.py, tests/test_smnist_gpu.py), rebuilt from seeds; shared so that
the fixture (tests/golden/smnist.npz, written by tests/make_golden_smnist.py from the reference's own sampler), the NumPy-driven restatement
(tests/smnist_ref.py), the host build of csrc/vs_mmnist_walk_core.h and the kernel see the same states and the same calls.  A case is a
start state (the key of RandomState(seed), `pos` set by hand), a geometry, the number of prefix draws and a list of calls, each a number of
trajectories; with fewer than four prefix draws every call also has its table of start states."""
import functools
import os
import struct
import subprocess

import numpy as np

import host_build
import smnist_ref
from mmnist_draws_inputs import N, ROOT, STATE_WORDS, random_state_at, start_state, state_words

START_POSITIONS = (0, 1, 227, 396, 397, 600, 623, 624)       # the phase edges of the regeneration, both ends of a block, and near its end
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'smnist.npz')
TRAIN = dict(frame=64, digit=(28, 28), max_speed=4, seq_len=15, n_source=256)
FRAME_SETS = (('frames64', 64, 4321), ('frames32', 32, 99))  # (key, frame, seed): 3 items x 2 digits x 6 frames of the reference's __getitem__
FRAME_ITEMS, FRAME_DIGITS, FRAME_LEN, FRAME_COND = 3, 2, 6, 2


def geometry(c):
    """(cols of the prefix, x_max, y_max)."""
    x_max, y_max, s = c['frame'] - c['digit'][0], c['frame'] - c['digit'][1], c['max_speed']
    full = [(0, c['n_source']), (0, x_max + 1), (0, y_max + 1), (-s, s + 1), (-s, s + 1)]
    return full[5 - c['n_pre']:] if c['n_pre'] else [], x_max, y_max


def _case(name, seed, pos, calls, n_pre=5, **geom):
    c = dict(TRAIN, name=name, state=start_state(seed, pos), calls=[int(n) for n in calls], n_pre=n_pre)
    c.update(geom)
    c['starts'] = None
    if n_pre < 4:                                            # a start table per call: positions inside the frame, speeds inside the range
        _, x_max, y_max = geometry(c)
        rs, s = np.random.RandomState(seed + 1), c['max_speed']
        c['starts'] = [np.stack([rs.randint(0, x_max + 1, n), rs.randint(0, y_max + 1, n), rs.randint(-s, s + 1, n), rs.randint(-s, s + 1, n)],
                                axis=1).astype(np.int32).reshape(n, 4) for n in c['calls']]
    return c


@functools.lru_cache(maxsize=None)
def state_whose_first_trajectory_ends_on_624():
    """(seed, pos): the first training trajectory from there stops consuming exactly at pos == 624, inside the block it started in."""
    cols, x_max, y_max = geometry(dict(TRAIN, n_pre=5))
    for seed in range(200, 2000):
        for pos in range(596, 620):
            rs = random_state_at(start_state(seed, pos))
            smnist_ref.sample(rs.randint, 1, TRAIN['seq_len'], cols, x_max, y_max, TRAIN['max_speed'])
            words = state_words(rs)
            if int(words[N]) == N and np.array_equal(words[:N], start_state(seed, pos)[:N]):
                return seed, pos
    raise AssertionError('no such state')


@functools.lru_cache(maxsize=None)
def cases():
    """[case]; the arrays are shared and must not be written to."""
    out = [_case('start_pos_%d' % p, 300 + p, p, [6]) for p in START_POSITIONS]
    seed, pos = state_whose_first_trajectory_ends_on_624()
    out.append(_case('ends_on_624', seed, pos, [1]))
    out.append(_case('ends_on_624_then_goes_on', seed, pos, [1, 2]))
    out.append(_case('n0', 42, N, [0]))
    out.append(_case('n1', 42, N, [1]))
    out.append(_case('n6', 42, N, [6]))
    out.append(_case('n256', 42, N, [256]))
    out.append(_case('one_frame', 43, 610, [6], seq_len=1))
    out.append(_case('tight_T100', 63, 620, [8], frame=29, seq_len=100))            # 2 266 outputs from pos 620: past the first window
    out.append(_case('tight_T400', 45, 500, [3], frame=29, seq_len=400))            # one trajectory needs more than a window holds
    out.append(_case('train_T100', 46, 13, [8], seq_len=100))
    out.append(_case('tight_29', 47, 400, [40], frame=29, seq_len=50))
    out.append(_case('tight_16_12_7', 48, 200, [40], frame=16, digit=(12, 12), max_speed=7, seq_len=40))
    out.append(_case('frame_32', 49, 30, [20], frame=32, seq_len=100))
    out.append(_case('fast_40', 50, 620, [30], max_speed=40, seq_len=30))
    out.append(_case('rect_28x20', 51, 250, [20], frame=40, digit=(28, 20)))
    out.append(_case('rect_12x30', 52, 350, [20], frame=36, digit=(12, 30), max_speed=6))
    out.append(_case('max_speed_0', 53, 620, [6], max_speed=0))
    out.append(_case('single_source_digit', 54, 618, [6], n_source=1))
    out.append(_case('n_pre_4', 55, 615, [6], n_pre=4))
    out.append(_case('n_pre_0_start_table', 56, 612, [6], n_pre=0))
    out.append(_case('n_pre_0_start_table_tight', 57, 5, [9, 4], n_pre=0, frame=29, seq_len=50))
    out.append(_case('n_pre_0_max_speed_0', 58, 77, [5], n_pre=0, max_speed=0))      # consumes nothing at all
    out.append(_case('split_3_3', 59, 590, [3, 3]))
    out.append(_case('split_summed', 59, 590, [6]))
    for c in out:
        c['state'].setflags(write=False)
    assert len({c['name'] for c in out}) == len(out)
    return out


def case(name):
    return next(c for c in cases() if c['name'] == name)


class Watch:
    """What a case contains, gathered from the restatement's notes while NumPy drives it."""

    def __init__(self, rs):
        self.rs, self.at, self.max_passes, self.two_edge_passes, self.redraws_across_blocks, self.prefixes_across_blocks = rs, {}, 0, 0, 0, 0
        self.outputs = []                                     # per trajectory, the outputs it consumed

    def __call__(self, event, value):
        if event == 'edges':
            self.two_edge_passes += value >= 2
        elif event == 'passes':
            self.max_passes = max(self.max_passes, value)
        elif value > 0:
            self.at[event] = self.rs.get_state()[2]
        else:
            before, after = self.at[event], self.rs.get_state()[2]
            straddles = before < N and after < before         # some outputs of the old block, some of the new one
            if event == 'pre':
                self.outputs.append(0)
            self.outputs[-1] += after - before if after >= before else N - before + after        # (both brackets hold a few outputs at most)
            if event == 'redraw':
                self.redraws_across_blocks += straddles
            else:
                self.prefixes_across_blocks += straddles


def run_reference(c, make_sampler):
    """[(pre int32 [n, n_pre], trajectories int32 [n, T, 4])] per call and the final state words, from `make_sampler(rs, watch)` ->
    sampler(n, cols, x_max, y_max, start) -> (pre, trajectories)."""
    cols, x_max, y_max = geometry(c)
    rs = random_state_at(c['state'])
    watch = Watch(rs)
    sampler = make_sampler(rs, watch)
    calls = []
    for k, n in enumerate(c['calls']):
        pre, traj = sampler(c, n, cols, x_max, y_max, c['starts'][k] if c['starts'] else None)
        pre = np.asarray(pre, dtype=np.int32).reshape(n, c['n_pre'])
        traj = np.asarray(traj, dtype=np.int32).reshape(n, c['seq_len'], 4)
        pre.setflags(write=False)
        traj.setflags(write=False)
        calls.append((pre, traj))
    words = state_words(rs)
    words.setflags(write=False)
    return calls, words, watch


def _restatement(rs, watch):
    return lambda c, n, cols, x_max, y_max, start: smnist_ref.sample(rs.randint, n, c['seq_len'], cols, x_max, y_max, c['max_speed'], start, watch)


@functools.lru_cache(maxsize=None)
def numpy_results():
    """{name: (calls, final state words, watch)}: the restatement driven by NumPy's scalar randint."""
    return {c['name']: run_reference(c, _restatement) for c in cases()}


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def golden_results():
    """{name: (calls, final state words)} of the fixture; the states and geometries it was written for must be the cases' own."""
    g, out = golden(), {}
    for c in cases():
        name = c['name']
        assert np.array_equal(g[name + ':state'], c['state']), name
        assert list(g[name + ':geom']) == [c['frame'], c['digit'][0], c['digit'][1], c['max_speed'], c['seq_len'], c['n_source'], c['n_pre']], name
        assert list(g[name + ':calls']) == c['calls'], name
        pre, traj, at, calls = g[name + ':pre'], g[name + ':traj'], 0, []
        for n in c['calls']:
            calls.append((pre[at:at + n], traj[at:at + n]))
            at += n
        out[name] = (calls, g[name + ':final'])
    return out


def positions_of(traj):
    """[n, T, 4] -> the kernel's positions [T, n, 2] and latents [T, n, 4]."""
    lat = np.ascontiguousarray(np.transpose(traj, (1, 0, 2)))
    return np.ascontiguousarray(lat[:, :, :2]), lat


def desc_of(pre, nd):
    n = pre.shape[0]
    return np.concatenate([np.arange(n // nd, dtype=np.int32)[:, None], pre[:, 0].reshape(n // nd, nd)], axis=1)


def desc_nd(c):
    """The digits per video with which a case asks for `desc`, or 0."""
    return 2 if c['n_pre'] == 5 and all(n % 2 == 0 for n in c['calls']) else 0


def compile_host_check(tmp_path, lanes=False):
    """tests/host/mmnist_walk_host_check.cpp, the plain build (the core's one-lane form) or (lanes=True) the lanes form with threads as lanes.
    (exe, sanitized)."""
    return host_build.compile_host_check(tmp_path, 'mmnist_walk_host_check', ['-ffp-contract=off'] + (['-pthread', '-DVSW_HOST_LANES'] if lanes else []),
                                         [str(tmp_path / 'empty.out'), '1'], '_lanes' if lanes else '')


def run_host_check(exe, case_list, tmp_path, lanes=1, tag='cases'):
    """The host build on `case_list` -> {name: (statuses, [None | dict(pre, positions, latents, desc)] per call, final state words)}."""
    src, dst = str(tmp_path / ('%s_%d.bin' % (tag, lanes))), str(tmp_path / ('%s_%d.out' % (tag, lanes)))
    with open(src, 'wb') as f:
        f.write(struct.pack('<q', len(case_list)))
        for c in case_list:
            cols, x_max, y_max = geometry(c)
            lows = [a for a, _ in cols] + [0] * (5 - len(cols))
            highs = [b for _, b in cols] + [0] * (5 - len(cols))
            f.write(np.asarray(c['state'], dtype='<u4').tobytes())
            f.write(struct.pack('<8i5i5i', c['n_pre'], c['seq_len'], x_max, y_max, c['max_speed'], 1, desc_nd(c), len(c['calls']), *lows, *highs))
            for k, n in enumerate(c['calls']):
                f.write(struct.pack('<q', n))
                if c['n_pre'] < 4:
                    f.write(np.asarray(c['starts'][k], dtype='<i4').tobytes())
    r = subprocess.run([exe, src, dst, str(lanes)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    blob = open(dst, 'rb').read()
    (count,), at, out = struct.unpack_from('<q', blob, 0), 8, {}
    assert count == len(case_list)

    def take(shape):
        nonlocal at
        n = int(np.prod(shape))
        a = np.frombuffer(blob, dtype='<i4', count=n, offset=at).reshape(shape)
        at += 4 * n
        return a

    for c in case_list:
        statuses, calls, T, nd = [], [], c['seq_len'], desc_nd(c)
        for n in c['calls']:
            (status,) = struct.unpack_from('<i', blob, at)
            at += 4
            statuses.append(status)
            if status != 0:
                calls.append(None)
                continue
            calls.append(dict(pre=take((n, c['n_pre'])), positions=take((T, n, 2)), latents=take((T, n, 4)),
                              desc=take((n // nd, 1 + nd)) if nd else None))
        words = np.frombuffer(blob, dtype='<u4', count=STATE_WORDS, offset=at)
        at += 4 * STATE_WORDS
        out[c['name']] = (statuses, calls, words)
    assert at == len(blob)
    return out

"""The deterministic Moving-MNIST walker (csrc/vs_mmnist_bounce_core.h: what vs_moving_mnist_batch and vs_moving_mnist_testset walk with, and
the body of the stochastic sampler) compiled for the host, under sanitizers where they link, against oracle/mmnist_ref.py: rounded positions
AND speeds of every frame, exactly, for every start and every speed pair of small frames and every 23rd start of larger ones."""
import itertools
import struct
import subprocess

import numpy as np
import pytest

import host_build
from oracle import mmnist_ref

MAX_PASSES = 64                                              # VSW_MAX_PASSES
# (x_max, y_max, max_speed, seq_len, every n-th start); 13 is the largest speed any test of the project uses
SETS = ((1, 1, 13, 24, 1), (2, 3, 13, 24, 1), (5, 5, 13, 24, 1), (1, 36, 7, 40, 23), (12, 10, 7, 40, 23), (36, 36, 4, 100, 23))
N_TRAJECTORIES = 45243


def _group(x_max, y_max, seq_len, starts, t0=0):
    return dict(x_max=x_max, y_max=y_max, seq_len=seq_len, t0=t0, starts=np.asarray(starts, dtype=np.int32).reshape(-1, 4))


def _set(x_max, y_max, speed, seq_len, every):
    where = list(itertools.product(range(x_max + 1), range(y_max + 1)))[::every]
    speeds = list(itertools.product(range(-speed, speed + 1), repeat=2))
    return _group(x_max, y_max, seq_len, [(sx, sy, dx, dy) for sx, sy in where for dx, dy in speeds])


def _oracle(g):
    """int32 [n, seq_len, 4]: mmnist_ref.trajectory's loop, which also keeps the speed of every frame."""
    out = np.empty((len(g['starts']), g['seq_len'], 4), dtype=np.int32)
    for i, q in enumerate(g['starts']):
        sx, sy, dx, dy = (int(v) for v in q)
        for t in range(g['seq_len']):
            sx, sy, dx, dy = mmnist_ref.process_collision(sx, sy, dx, dy, g['x_max'], g['y_max'])
            out[i, t] = (int(round(sx)), int(round(sy)), dx, dy)
            sy += dy
            sx += dx
        if i % 50 == 0:
            assert [tuple(r) for r in out[i, :, :2]] == mmnist_ref.trajectory(*q, g['seq_len'], g['x_max'], g['y_max'])
    return out


def _run(exe, groups, tmp_path, tag):
    """[(gave_up int32 [n], rows int32 [n, seq_len - t0, 4])] per group, and the program's last line."""
    src, dst = str(tmp_path / (tag + '.bin')), str(tmp_path / (tag + '.out'))
    with open(src, 'wb') as f:
        f.write(struct.pack('<q', len(groups)))
        for g in groups:
            f.write(struct.pack('<5i', g['x_max'], g['y_max'], g['seq_len'], g['t0'], len(g['starts'])) + g['starts'].astype('<i4').tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    blob, at, out = open(dst, 'rb').read(), 8, []
    assert struct.unpack_from('<q', blob, 0) == (len(groups),)
    for g in groups:
        n, rows = len(g['starts']), g['seq_len'] - g['t0']
        a = np.frombuffer(blob, dtype='<i4', count=n * (1 + rows * 4), offset=at).reshape(n, 1 + rows * 4)
        at += a.nbytes
        out.append((a[:, 0], a[:, 1:].reshape(n, rows, 4)))
    assert at == len(blob)
    return out, r.stdout.strip().splitlines()[-1]


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path, sanitized = host_build.compile_host_check(tmp_path_factory.mktemp('bounce'), 'mmnist_bounce_host_check', ['-ffp-contract=off'],
                                                    [str(tmp_path_factory.mktemp('bounce_start') / 'empty.out')])
    print('sanitizers:', sanitized)
    return path


def test_walker_equals_the_oracle_on_every_start_and_speed(exe, tmp_path):
    groups = [_set(*s) for s in SETS]
    # a digit that fills the frame along one axis and does not move along it, and the mirror image
    groups.append(_group(0, 5, 24, [(0, sy, 0, dy) for sy in range(6) for dy in range(-13, 14)]))
    groups.append(_group(5, 0, 24, [(sx, 0, dx, 0) for sx in range(6) for dx in range(-13, 14)]))
    assert sum(len(g['starts']) for g in groups[:len(SETS)]) == N_TRAJECTORIES
    got, line = _run(exe, groups, tmp_path, 'sets')
    print(line)
    for g, (gave_up, rows) in zip(groups, got):
        want = _oracle(g)
        assert not gave_up.any(), (g['x_max'], g['y_max'])              # no trajectory ends on the pass budget: none may be skipped
        assert rows.shape == want.shape
        bad = np.nonzero((rows != want).any(axis=(1, 2)))[0]
        assert len(bad) == 0, (g['x_max'], g['y_max'], len(bad), g['starts'][bad[0]], rows[bad[0]][:6], want[bad[0]][:6])
        assert rows[..., 0].min() >= 0 and rows[..., 0].max() <= g['x_max'] and rows[..., 1].min() >= 0 and rows[..., 1].max() <= g['y_max']


def test_frames_before_the_chunk_are_replayed_not_recorded(exe, tmp_path):
    whole = _set(5, 5, 13, 24, 7)
    (_, rows), (_, late), (_, last) = _run(exe, [whole, dict(whole, t0=7), dict(whole, t0=23)], tmp_path, 'chunks')[0]
    assert late.shape[1] == 17 and np.array_equal(late, rows[:, 7:]) and np.array_equal(last, rows[:, 23:])


def test_past_the_pass_budget_the_walker_terminates_inside_its_rows(exe, tmp_path):
    """x_max = 1 and a row speed of 200: a pass mirrors the position about a border, which brings it 2 nearer, so a frame needs about 100
    passes > VSW_MAX_PASSES.  No oracle (the walker gives up where the reference goes on): it ends, the sanitizers stay silent, and the
    recorded positions are within one pixel of the frame (vsw_round)."""
    assert 200 / 2 > MAX_PASSES
    g = _group(1, 5, 3000, [(0, 2, 200, 3), (1, 0, -200, 0), (0, 5, 200, -7)])
    (gave_up, rows), = _run(exe, [g], tmp_path, 'budget')[0]
    assert (gave_up > 0).all()
    assert rows[..., 0].min() >= -1 and rows[..., 0].max() <= 2 and rows[..., 1].min() >= -1 and rows[..., 1].max() <= 6

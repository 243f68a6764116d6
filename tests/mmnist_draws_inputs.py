"""Cases of the device-side NumPy stream's tests (tests/test_mmnist_draws_cpu.py, tests/test_mmnist_draws_gpu.py), rebuilt from seeds; shared so
that NumPy, the host build of csrc/vs_mt19937_core.h and the kernel see the same states and the same calls.  A case is a start state (the key
of RandomState(seed), `pos` set by hand: every key / pos pair is a state of the stream), up to 8 columns (low, high) and a list of calls, each
a number of rows; the oracle is NumPy itself: set_state, then the scalar randint calls in order."""
import functools
import os
import struct
import subprocess

import numpy as np

import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STATE_WORDS, MAX_COLS = 624, 625, 8
START_POSITIONS = (0, 1, 227, 396, 397, 623, 624)          # the phase edges of the regeneration and both ends of a block
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def product_cols(n_source=256, frame=64, h=28, w=28, speed=4):
    """The five columns of MovingMNIST.draw: digit index, start row, start column, row speed, column speed."""
    return [(0, n_source), (0, frame - h + 1), (0, frame - w + 1), (-speed, speed + 1), (-speed, speed + 1)]


def start_state(seed, pos):
    """uint32 [625]: the key of RandomState(seed) and `pos`."""
    words = np.empty(STATE_WORDS, dtype=np.uint32)
    words[:N] = np.random.RandomState(seed).get_state()[1]
    words[N] = pos
    return words


def random_state_at(words):
    rs = np.random.RandomState(0)
    rs.set_state(('MT19937', np.asarray(words[:N], dtype=np.uint32), int(words[N])))
    return rs


def state_words(rs):
    st = rs.get_state()
    return np.concatenate([np.asarray(st[1], dtype=np.uint32), np.array([st[2]], dtype=np.uint32)])


@functools.lru_cache(maxsize=None)
def rows_that_end_on_624(seed=11, pos=300):
    """The number of rows of the product's columns after which NumPy's pos is exactly 624, for the first time and still inside the block the
    case starts in, found by stepping NumPy; the seed is moved on until there is one."""
    while True:
        rs = random_state_at(start_state(seed, pos))
        for rows in range(1, 80):
            for low, high in product_cols():
                rs.randint(low, high)
            at = rs.get_state()[2]
            if at == N:
                return seed, rows
            if at < pos:                                    # the block was left without landing on its end
                break
        seed += 1


def _case(name, seed, pos, cols, calls):
    return dict(name=name, state=start_state(seed, pos), cols=[(int(a), int(b)) for a, b in cols], calls=[int(r) for r in calls])


@functools.lru_cache(maxsize=None)
def cases():
    """[case]; the arrays are shared and must not be written to."""
    out = [_case('start_pos_%d' % p, 100 + p, p, product_cols(), [40]) for p in START_POSITIONS]
    seed, rows = rows_that_end_on_624()
    out.append(_case('ends_on_624', seed, 300, product_cols(), [rows]))
    out.append(_case('ends_on_624_then_goes_on', seed, 300, product_cols(), [rows, 3]))
    out.append(_case('two_regenerations', 21, 10, [(0, 1 << 16)], [1300]))
    for b, nd in ((1, 1), (3, 2), (128, 2)):
        out.append(_case('product_B%d_nd%d' % (b, nd), 42, N, product_cols(), [b * nd]))
    out.append(_case('product_mnist_60000', 43, 17, product_cols(n_source=60000), [64]))
    out.append(_case('rng0_alone', 51, 5, [(5, 6)], [7]))
    out.append(_case('rng0_mixed_in', 52, 600, [(0, 37), (5, 6), (-4, 5), (0, 1)], [50]))
    out.append(_case('rng0_first_and_last', 53, 100, [(-7, -6), (0, 9), (3, 4)], [300]))
    out.append(_case('rng0_every_column', 54, 620, [(5, 6), (0, 1), (-3, -2)], [9]))
    out.append(_case('frame_equals_digit_height_zero_speed', 55, 400, [(0, 20), (0, 1), (0, 13), (0, 1), (-4, 5)], [24]))
    out.append(_case('never_rejects', 61, 500, [(0, 2), (0, 32), (0, 65536), (-8, 8)], [100]))
    out.append(_case('rejects_half', 62, 500, [(0, 3), (0, 33), (0, 65537), (-16, 17)], [100]))
    out.append(_case('negative_lows', 63, 0, [(-100, -3), (I32_MIN, I32_MIN + 10), (-1, 1)], [50]))
    out.append(_case('k1', 64, 380, [(0, 37)], [300]))
    out.append(_case('k8', 65, 390, [(0, 256), (0, 37), (-4, 5), (0, 3), (10, 1000), (-5, 6), (0, 2), (7, 70000)], [100]))
    out.append(_case('wide_full', 66, 200, [(I32_MIN, I32_MAX)], [100]))
    out.append(_case('wide_positive', 67, 200, [(0, I32_MAX)], [100]))
    out.append(_case('wide_mixed', 68, 610, [(I32_MIN, I32_MAX), (0, 37), (0, I32_MAX), (I32_MIN, 0), (-1, I32_MAX)], [60]))
    out.append(_case('back_to_back', 71, 250, product_cols(), [5, 11, 300]))
    out.append(_case('back_to_back_summed', 71, 250, product_cols(), [316]))
    out.append(_case('zero_rows', 72, 30, product_cols(), [0, 4, 0]))
    for c in out:
        c['state'].setflags(write=False)
    assert len({c['name'] for c in out}) == len(out)
    return out


def case(name):
    return next(c for c in cases() if c['name'] == name)


@functools.lru_cache(maxsize=None)
def numpy_results():
    """{name: (tables, final state words)}: per call the int64 [rows, k] table of NumPy's scalar randint calls, in order."""
    out = {}
    for c in cases():
        rs = random_state_at(c['state'])
        tables = []
        for rows in c['calls']:
            t = np.array([[rs.randint(low, high) for low, high in c['cols']] for _ in range(rows)], dtype=np.int64).reshape(rows, len(c['cols']))
            t.setflags(write=False)
            tables.append(t)
        words = state_words(rs)
        words.setflags(write=False)
        out[c['name']] = (tables, words)
    return out


def compile_host_check(tmp_path, lanes=False):
    """tests/host/mt19937_host_check.cpp, the plain build or (lanes=True) the one in which threads play the lanes.  (exe, sanitized)."""
    return host_build.compile_host_check(tmp_path, 'mt19937_host_check', ['-pthread', '-DVSM_HOST_LANES'] if lanes else [],
                                         [str(tmp_path / 'empty.out'), '1'], '_lanes' if lanes else '')


def run_host_check(exe, case_list, tmp_path, lanes=1, tag='cases'):
    """The host build on `case_list` -> {name: (statuses, tables, final state words)}."""
    src, dst = str(tmp_path / ('%s_%d.bin' % (tag, lanes))), str(tmp_path / ('%s_%d.out' % (tag, lanes)))
    with open(src, 'wb') as f:
        f.write(struct.pack('<q', len(case_list)))
        for c in case_list:
            k = len(c['cols'])
            lows = [a for a, _ in c['cols']] + [0] * (MAX_COLS - k)
            highs = [b for _, b in c['cols']] + [0] * (MAX_COLS - k)
            f.write(np.asarray(c['state'], dtype='<u4').tobytes() + struct.pack('<i8i8ii', k, *lows, *highs, len(c['calls'])))
            f.write(struct.pack('<%dq' % len(c['calls']), *c['calls']))
    r = subprocess.run([exe, src, dst, str(lanes)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    blob = open(dst, 'rb').read()
    (count,), at, out = struct.unpack_from('<q', blob, 0), 8, {}
    assert count == len(case_list)
    for c in case_list:
        k, statuses, tables = len(c['cols']), [], []
        for rows in c['calls']:
            (status,) = struct.unpack_from('<i', blob, at)
            at += 4
            statuses.append(status)
            if status == 0:
                tables.append(np.frombuffer(blob, dtype='<i4', count=rows * k, offset=at).reshape(rows, k))
                at += 4 * rows * k
            else:
                tables.append(None)
        words = np.frombuffer(blob, dtype='<u4', count=STATE_WORDS, offset=at)
        at += 4 * STATE_WORDS
        out[c['name']] = (statuses, tables, words)
    assert at == len(blob)
    return out

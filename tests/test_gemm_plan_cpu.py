"""The GEMM planner (csrc/vs_gemm_plan.h) through the host-only entry point vs_gemm_plan: no GPU.

tests/golden/gemm_plans.npz (tests/make_golden_gemm_plans.py) records, for a grid of shapes, batches, compute types, layouts, operand
alignments and switch settings, which tile kernel ran and in how many K splits BEFORE the planners moved into one header; a change that
means to move a decision regenerates the table and shows which rows moved.
"""
import ctypes
import json

import numpy as np
import pytest

from make_golden_gemm_plans import BF16, COLS, KIND, PATH, evaluate, operand, switches


@pytest.fixture(scope='module')
def lib():
    from spatiotemporal_variable_separation_amd import _lib
    _lib.build_library()
    return _lib.load_library()


@pytest.fixture(scope='module')
def replay(lib):
    table = np.load(PATH)
    plans, workspace = evaluate(lib, table['inputs'], json.loads(str(table['env_sets'])))
    return table, plans, workspace


def test_every_recorded_plan_reproduces(replay):
    table, plans, _ = replay
    assert len(table['inputs']) > 60000
    bad = np.nonzero((plans != table['plans']).any(axis=1))[0]
    assert len(bad) == 0, [(table['inputs'][i].tolist(), dict(zip(COLS, table['plans'][i].tolist())), dict(zip(COLS, plans[i].tolist())))
                           for i in bad[:5]]


def test_workspace_bounds_equal_the_recorded_ones(replay):
    table, _, workspace = replay
    bad = np.nonzero((workspace != table['workspace']).any(axis=1))[0]
    assert len(bad) == 0, [(table['inputs'][i].tolist(), table['workspace'][i].tolist(), workspace[i].tolist()) for i in bad[:5]]
    # the bound covers what any single call needs
    assert (table['workspace'][:, 1] >= table['plans'][:, 11]).all()


def _plan(lib, M, N, K, **env):
    out = (ctypes.c_int64 * len(COLS))()
    a, lda, sa = operand(M, K, 0)
    b, ldb, sb = operand(N, K, 0)
    with switches(env):
        assert lib.vs_gemm_plan(BF16, 1, M, N, K, a, lda, sa, 0, b, ldb, sb, 0, out) == 0
    return dict(zip(COLS, out))


def test_named_decisions(lib):
    """bf16, aligned R x R operands, one problem: the policy a reader should know."""
    def check(shape, kind, **want):
        env = {k: want.pop(k) for k in list(want) if k.startswith('VS_')}
        p = _plan(lib, *shape, **env)
        assert p['kind'] == KIND[kind] and all(p[k] == v for k, v in want.items()), (shape, kind, want, p)
    check((3328, 4096, 1200), 'P8', ni=2, splits=1)
    check((3328, 1200, 4096), 'P8', ni=1)
    check((3328, 1200, 1200), 'P8', ni=1)
    check((4096, 1200, 3328), 'P8', ni=1)
    check((256, 1200, 20480), 'P8', ni=1, splits=25)
    check((1200, 1200, 3328), 'MID', splits=4)
    check((128, 1200, 20480), 'MID', splits=32)
    check((4096, 4096, 4096), 'P8', ni=2)
    check((4096, 4096, 4096), 'GLDS', VS_GEMM_P8='0', VS_GEMM_BIG='0')
    check((64, 64, 64), 'REG', bm=64, bn=64, splits=1)
    assert lib.vs_gemm_workspace_bytes(128, 1200, 20480) > 0
    assert lib.vs_gemm_workspace_bytes(4096, 4096, 4096) == 0

"""Generate tests/golden/gemm_plans.npz: which tile kernel, in how many K splits, vs_gemm / vs_gemm_batched take for a grid of problems
(the host-only entry point vs_gemm_plan) and the workspace bounds of the same problems.

TEST INFRASTRUCTURE ONLY; needs the built library, no GPU:

    python tests/make_golden_gemm_plans.py

The committed table was written by the planners as they stood BEFORE they moved into csrc/vs_gemm_plan.h (vs_gemm_plan added on top of the
four per-header planners, nothing else changed), so tests/test_gemm_plan_cpu.py checks the refactor against the old rules and every later
tuning change shows which problems changed kernel.  Regenerate it only with a change that means to move a decision.

Arrays: `inputs` [cases, 14] = compute, batch, M, N, K, address of A, lda, stride_a, layout_a, address of B, ldb, stride_b, layout_b,
index into `env_sets`;  `plans` [cases, 12] = what vs_gemm_plan fills;  `workspace` [cases, 2] = vs_gemm_workspace_bytes(M, N, K),
vs_gemm_batched_workspace_bytes(batch, M, N, K);  `env_sets` = JSON list of the switch settings a case runs under.
"""
import contextlib
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
PATH = os.path.join(HERE, 'golden', 'gemm_plans.npz')

F32, BF16 = 0, 1
KIND = {'REG': 0, 'GLDS': 1, 'MID': 2, 'BIG': 3, 'P8': 4}
COLS = ('kind', 'bm', 'bn', 'splits', 'k_tiles_per_split', 'tiles_m', 'tiles_n', 'stages', 'ni', 'mi', 'fused', 'slab_bytes')
SWITCHES = ('VS_GEMM_TILE', 'VS_GEMM_BIG', 'VS_GEMM_MID', 'VS_GEMM_P8', 'VS_GEMM_P8_NI', 'VS_GEMM_P8_MI')
# the settings the GPU tests of tests/test_gemm_gpu.py run their named shapes under (index 0: nothing set)
ENV_SETS = [{},
            {'VS_GEMM_BIG': '2', 'VS_GEMM_P8': '0'},
            {'VS_GEMM_MID': '2', 'VS_GEMM_BIG': '0', 'VS_GEMM_P8': '0'},
            {'VS_GEMM_MID': '1', 'VS_GEMM_BIG': '0', 'VS_GEMM_P8': '0'},
            {'VS_GEMM_P8': '2', 'VS_GEMM_P8_NI': '2', 'VS_GEMM_P8_MI': '4'},
            {'VS_GEMM_P8': '2', 'VS_GEMM_P8_NI': '1', 'VS_GEMM_P8_MI': '4'},
            {'VS_GEMM_P8': '2', 'VS_GEMM_P8_NI': '1', 'VS_GEMM_P8_MI': '2'},
            {'VS_GEMM_TILE': '128x128'},
            {'VS_GEMM_P8': '0', 'VS_GEMM_BIG': '0'}]
BASE = 1 << 20          # operand addresses are looked at for alignment only


@contextlib.contextmanager
def switches(env):
    """The GEMM planner switches set to exactly `env` (they are read per call); the caller's values come back afterwards."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def operand(rows, K, layout, misalign=None):
    """(address, ld, batch stride) of a [rows, K] operand: 'addr' = not 16-byte aligned, 'ld' = leading dimension no multiple of 8."""
    ld = -(-(K if layout == 0 else rows) // 8) * 8 + (4 if misalign == 'ld' else 0)
    return BASE + (2 if misalign == 'addr' else 0), ld, ld * (rows if layout == 0 else K)


def case(compute, batch, M, N, K, la, lb, env=0, mis_a=None, mis_b=None):
    return (compute, batch, M, N, K) + operand(M, K, la, mis_a) + (la,) + operand(N, K, lb, mis_b) + (lb, env)


def cases():
    from test_gemm_gpu import BIG_SHAPES, MID_SHAPES, P8_SHAPES, SHAPES, SPLITK_SHAPES
    mn = (32, 64, 65, 128, 129, 256, 257, 512, 1000, 1200, 2048, 3328, 4096, 8192)
    ks = (64, 256, 512, 520, 1200, 3328, 4096, 20480, 65536)
    rows = []
    for compute in (F32, BF16):
        for batch in (1, 3, 24):
            for M in mn:
                for N in mn:
                    for K in ks:
                        for lay in (0, 1):
                            rows.append(case(compute, batch, M, N, K, lay, lay))
                            rows.append(case(compute, batch, M, N, K, lay, lay, mis_a='addr'))
                            rows.append(case(compute, batch, M, N, K, lay, lay, mis_b='ld'))
    named = sorted(set(SHAPES + BIG_SHAPES + MID_SHAPES + SPLITK_SHAPES + P8_SHAPES + [(4096, 4096, 4096), (64, 64, 64), (128, 1200, 20480)]))
    for env in range(len(ENV_SETS)):
        for compute in (F32, BF16):
            for batch in (1, 3):
                for (M, N, K) in named:
                    for la in (0, 1):
                        for lb in (0, 1):
                            rows.append(case(compute, batch, M, N, K, la, lb, env))
    return np.array(rows, dtype=np.int64)


def evaluate(lib, inputs, env_sets):
    """(plans, workspace) of every row of `inputs`, each under its switch setting."""
    plans = np.zeros((len(inputs), len(COLS)), dtype=np.int64)
    workspace = np.zeros((len(inputs), 2), dtype=np.int64)
    out = (ctypes.c_int64 * len(COLS))()
    for e, env in enumerate(env_sets):
        with switches(env):
            for i in np.nonzero(inputs[:, 13] == e)[0]:
                compute, batch, M, N, K, a, lda, sa, la, b, ldb, sb, lb = (int(v) for v in inputs[i, :13])
                rc = lib.vs_gemm_plan(compute, batch, M, N, K, a, lda, sa, la, b, ldb, sb, lb, out)
                assert rc == 0, (rc, lib.vs_last_error())
                plans[i] = out[:]
                workspace[i] = lib.vs_gemm_workspace_bytes(M, N, K), lib.vs_gemm_batched_workspace_bytes(batch, M, N, K)
    return plans, workspace


def main():
    from spatiotemporal_variable_separation_amd import _lib
    _lib.build_library()
    inputs = cases()
    plans, workspace = evaluate(_lib.load_library(), inputs, ENV_SETS)
    col = np.asfortranarray          # stored column by column: a column varies slowly, the file is a tenth of the row-major one
    np.savez_compressed(PATH, inputs=col(inputs), plans=col(plans), workspace=col(workspace), env_sets=np.array(json.dumps(ENV_SETS)))
    print('wrote', PATH, len(inputs), 'cases,', os.path.getsize(PATH), 'bytes; kinds:',
          {k: int((plans[:, 0] == v).sum()) for k, v in KIND.items()})


if __name__ == '__main__':
    main()

"""The addressing contract of vs_gemm / vs_gemm_batched on every tile family: leading dimensions larger than the extent, operands and outputs
that start inside a larger buffer, pointers off 16-byte alignment, and nothing written outside the output window.

Operands are embedded in all-NaN buffers (tests/guard_util.py), so a K-tail or row-tail read that strays into the padding poisons the result;
outputs are windows of all-0xFF buffers that are checked byte by byte after every call.  Every case first asks the planner (vs_gemm_plan,
with the very pointers and leading dimensions of the case, under the case's switches) which family runs it and asserts the intended one.

Oracle: the fp64 contraction of the same rounded operands, with the bounds of tests/test_gemm_gpu.py (2e-6 relative L2 for fp32 results,
3e-6 with an activation or a mask, 6e-3 / 8e-4 for one bf16 / fp16 rounding of the result).  Where the planner returns the same row for the
strided call and for the dense call of the same problem, the two results are also bit-equal: same kernel, same summation order.
"""
import ctypes
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
REG, GLDS, MID, BIG, P8 = 0, 1, 2, 3, 4

_P8 = dict(VS_GEMM_P8='2')
FAMILIES = {
    # name: (kind, switches as test_gemm_gpu.py sets them, shapes, compute types)
    'reg': (REG, {}, [(100, 70, 50), (33, 200, 20)], [F32, BF16, F16]),
    'glds': (GLDS, dict(VS_GEMM_GLDS='2', VS_GEMM_TILE='128x128'), [(128, 136, 72), (300, 200, 200)], [BF16, F16]),      # (one child process)
    'mid': (MID, dict(VS_GEMM_MID='2', VS_GEMM_BIG='0', VS_GEMM_P8='0'), [(136, 264, 40)], [BF16, F16]),
    'big': (BIG, dict(VS_GEMM_BIG='2', VS_GEMM_P8='0'), [(520, 2048, 776)], [BF16, F16]),
    'p8-2': (P8, dict(_P8, VS_GEMM_P8_NI='2', VS_GEMM_P8_MI='4'), [(264, 520, 136)], [BF16, F16]),
    'p8-1': (P8, dict(_P8, VS_GEMM_P8_NI='1', VS_GEMM_P8_MI='4'), [(264, 520, 136)], [BF16, F16]),
    'p8-1m2': (P8, dict(_P8, VS_GEMM_P8_NI='1', VS_GEMM_P8_MI='2'), [(264, 520, 136)], [BF16, F16]),
}
SPLITK_SHAPES = [(100, 70, 4104), (256, 32, 1200)]
WINDOWS = ('aligned', 'general')


def _window_form(form, N):
    """(ldc, element offset) of an output window that begins at row 1 of its buffer.
    'aligned': ldc = N + 12, offset 4 -- with N % 8 == 0 (every DMA-family shape) row 1 starts 16-byte aligned, ldc % 4 == 0 and N % 4 == 0:
               every condition of the fast epilogues holds.
    'general': ldc = N + 13, C off 16-byte alignment.  An offset of 3 puts row 1 back ON a 16-byte boundary whenever N % 8 == 0
               (3 + N + 13 = N + 16), so the offset is the one of 3 and 4 that makes (offset + ldc) odd: misaligned for 2- and 4-byte elements."""
    if form == 'aligned':
        return N + 12, 4
    return N + 13, 3 if (3 + N + 13) % 2 else 4


def _window(form, M, N, dtype, batch=None):
    from guard_util import window
    ldc, off = _window_form(form, N)
    shape, kw = ((M, N), {}) if batch is None else ((batch, M, N), dict(batch_stride=M * ldc + 8))
    c, g = window(shape, dtype, ld=ldc, offset=off, device='cuda', rows_before=1, rows_after=1, **kw)
    assert c.stride(-2) == ldc and (c.data_ptr() % 16 == 0) == (form == 'aligned' and N % 8 == 0), (form, N, dtype, c.data_ptr() % 16)
    return c, g
EPILOGUES = ('plain', 'bias_relu', 'mask', 'mask_off', 'accumulate', 'bias_off')


class _Env:
    def __init__(self, kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _tol(out_dtype, activated):
    return {BF16: 6e-3, F16: 8e-4}.get(out_dtype, 3e-6 if activated else 2e-6)


def _rel(got, ref):
    """Relative L2 error; NaN (an element never written, or padding that was read) compares as a failure."""
    err = ((got.double() - ref).norm() / ref.norm()).item()
    return err if err == err else float('inf')


@functools.lru_cache(maxsize=None)
def _problem(M, N, K, dtype):
    """Rounded operands a [M, K], b [N, K] on the device, and everything the epilogues need with its fp64 reference (computed once per problem)."""
    from oracle.detdata import det_uniform
    a = ((det_uniform((M, K), 3) - 0.5) * 2.0).to(dtype)
    b = ((det_uniform((N, K), 5) - 0.5) * 2.0).to(dtype)
    bias = (det_uniform((N + 1,), 9) - 0.5) * 0.5                       # bias_buf: [1:] is the misaligned bias vector
    mask = (det_uniform((M, N), 31) - 0.3).to(dtype if dtype != F32 else F32)
    prev = det_uniform((M, N), 33)
    c = a.double() @ b.double().t()
    ref = {'plain': c, 'bias_relu': torch.relu(c + bias[:N].double()), 'bias_off': c + bias[1:].double(),
           'mask': 0.5 * c * torch.where(mask.double() > 0, 1.0, 0.2)}
    ref['mask_off'] = ref['mask']
    return dict(a=a.cuda(), b=b.cuda(), bias=bias.cuda(), mask=mask.cuda(), prev=prev, c=c.cuda(), ref={k: v.cuda() for k, v in ref.items()})


def _form(x, layout):
    """[rows, K] -> the matrix as the layout stores it (R: [rows, K]; S: [K, rows])."""
    return x if layout == 0 else x.t().contiguous()


def _plan(dtype, M, N, K, a, la, b, lb, batch=1, lda=None, ldb=None, stride_a=0, stride_b=0):
    from spatiotemporal_variable_separation_amd import _lib
    out = (ctypes.c_int64 * 12)()
    lda = a.stride(-2) if lda is None else lda
    ldb = b.stride(-2) if ldb is None else ldb
    _lib.check(_lib.load_library().vs_gemm_plan(_lib.code_of(dtype), batch, M, N, K, a.data_ptr(), lda, stride_a, la, b.data_ptr(), ldb, stride_b, lb,
                                                out), 'vs_gemm_plan')
    return list(out)


def _fits(ptr, ld, layout, rows, K, batch_stride=0):
    """The operand condition of the LDS-DMA loaders as include/varsep_hip.h states it (16-byte base, multiples of 8)."""
    return ptr % 16 == 0 and ld % 8 == 0 and batch_stride % 8 == 0 and (K % 8 == 0 if layout == 0 else rows % 8 == 0)


def _expected_kind(kind, dtype, M, N, K, a, la, b, lb):
    if kind == REG or dtype == F32:
        return REG
    return kind if _fits(a.data_ptr(), a.stride(0), la, M, K) and _fits(b.data_ptr(), b.stride(0), lb, N, K) else REG


def _epilogue_call(ops, p, epi, a, la, b, lb, M, N, K, out_dtype, out=None, embed=None):
    """One ops.gemm with the epilogue `epi`; `out` None: a dense result (the comparator).  Returns (result, guards of the embedded mask)."""
    kw, guards = {}, []
    if epi == 'bias_relu':
        kw = dict(bias=p['bias'][:N], act='relu')
    elif epi == 'bias_off':
        kw = dict(bias=p['bias'][1:])
        assert kw['bias'].data_ptr() % 16 == 4 and kw['bias'].is_contiguous()
    elif epi in ('mask', 'mask_off'):
        mask = p['mask']
        if out is not None:
            mask, g = embed(p['mask'], ld=N + (4 if epi == 'mask' else 5), offset=0 if epi == 'mask' else 1)
            assert (mask.data_ptr() % 16 == 0) == (epi == 'mask')
            guards.append(g)
        kw = dict(alpha=0.5, mask=mask, mask_act='leaky_relu')
    elif epi == 'accumulate':
        if out is None:
            out = p['prev'].to(out_dtype).cuda()
        else:
            out.copy_(p['prev'].to(out_dtype))
        kw = dict(accumulate=True)
    return ops.gemm(a, la, b, lb, M, N, K, out=out, out_dtype=out_dtype, **kw), guards


def _epilogue_ref(p, epi, out_dtype):
    if epi == 'accumulate':
        return p['prev'].to(out_dtype).double().cuda() + p['c']
    return p['ref'][epi]


def _check_family(name, dtype, la, lb, shapes=None):
    """Cases a (padded operands that fit), b (output windows x epilogues) and c (one loader condition violated) of one family."""
    from guard_util import embed, window
    from spatiotemporal_variable_separation_amd import ops
    kind, env, fam_shapes, _ = FAMILIES[name]
    out16 = dtype if dtype != F32 else BF16
    with _Env(env):
        for si, (M, N, K) in enumerate(shapes or fam_shapes):
            what = '%s %s (%d,%d) %dx%dx%d' % (name, dtype, la, lb, M, N, K)
            p = _problem(M, N, K, dtype)
            ext_a, ext_b = (K if la == 0 else M), (K if lb == 0 else N)
            ad, bd = _form(p['a'], la), _form(p['b'], lb)
            dense_plan = _plan(dtype, M, N, K, ad, la, bd, lb)
            if si == 0:                                                  # the family's first shape fits its loader in every layout
                assert dense_plan[0] == kind, (what, dense_plan)

            # ---- a. padded operands that still fit the DMA loader: NaN behind every row and in front of the first
            a, ga = embed(ad, ld=ext_a + 24, offset=8)
            b, gb = embed(bd, ld=ext_b + 8, offset=8)
            assert a.stride(0) == ext_a + 24 and b.stride(0) == ext_b + 8 and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
            plan = _plan(dtype, M, N, K, a, la, b, lb)
            assert plan[0] == _expected_kind(kind, dtype, M, N, K, a, la, b, lb) == dense_plan[0], (what, plan, dense_plan)
            dense = {}
            for od in (F32, out16):
                for epi in EPILOGUES:
                    if epi != 'mask_off':
                        dense[od, epi], _ = _epilogue_call(ops, p, epi, ad, la, bd, lb, M, N, K, od)
                dense[od, 'mask_off'] = dense[od, 'mask']
            got = ops.gemm(a, la, b, lb, M, N, K)
            assert _rel(got, p['c']) < _tol(F32, False), (what, 'padded operands', _rel(got, p['c']))
            assert _rel(dense[F32, 'plain'], p['c']) < _tol(F32, False), (what, 'dense', _rel(dense[F32, 'plain'], p['c']))
            if plan == dense_plan:
                assert torch.equal(got, dense[F32, 'plain']), (what, 'padded operands differ from the dense call')

            # ---- b. output windows at row 1 of an (M + 2)-row buffer, both alignments, fp32 and 16-bit results, every epilogue
            for form in WINDOWS:
                for od in (F32, out16):
                    for epi in EPILOGUES:
                        c, gc = _window(form, M, N, od)
                        _, gm = _epilogue_call(ops, p, epi, a, la, b, lb, M, N, K, od, out=c, embed=embed)
                        case = (what, form, od, epi)
                        gc.check()
                        for g in gm + [ga, gb]:
                            g.check()
                        err = _rel(c, _epilogue_ref(p, epi, od))
                        assert err < _tol(od, epi != 'plain' and epi != 'accumulate'), (case, err)
                        if plan == dense_plan:
                            assert torch.equal(c, dense[od, epi]), (case, 'differs from the dense call')

            # ---- c. operands that do NOT fit: one condition of the loader at a time, on A and on B -> the register tile, and right numbers
            for which in ('a', 'b'):
                for viol in ('ld', 'offset', 'extent'):
                    m, n, k = M, N, K
                    if viol == 'extent':                                 # R: K not a multiple of 8; S: rows not a multiple of 8 (4 less, where it is one)
                        lay = la if which == 'a' else lb
                        if lay == 0:
                            k = K - 4 if K % 8 == 0 else K
                        elif which == 'a':
                            m = M - 4 if M % 8 == 0 else M
                        else:
                            n = N - 4 if N % 8 == 0 else N
                    a2, b2 = _form(p['a'][:m, :k], la), _form(p['b'][:n, :k], lb)
                    pads = {'a': dict(ld=a2.shape[1]), 'b': dict(ld=b2.shape[1])}
                    if viol == 'ld':
                        pads[which]['ld'] += 1
                    elif viol == 'offset':
                        pads[which]['offset'] = 1
                    a2, ga2 = embed(a2, **pads['a'])
                    b2, gb2 = embed(b2, **pads['b'])
                    if dtype != F32:
                        assert not (_fits(a2.data_ptr(), a2.stride(0), la, m, k) and _fits(b2.data_ptr(), b2.stride(0), lb, n, k)), (what, which, viol)
                    plan2 = _plan(dtype, m, n, k, a2, la, b2, lb)
                    assert plan2[0] == REG, (what, which, viol, plan2)
                    c, gc = window((m, n), F32, ld=n + 1, offset=1, device='cuda', rows_before=1)
                    ops.gemm(a2, la, b2, lb, m, n, k, out=c)
                    gc.check()
                    ref = p['a'][:m, :k].double() @ p['b'][:n, :k].double().t()
                    assert _rel(c, ref) < _tol(F32, False), (what, which, viol, _rel(c, ref))


@pytest.mark.parametrize('la,lb', LAYOUTS)
@pytest.mark.parametrize('name,dtype', [(n, dt) for n in FAMILIES if n != 'glds' for dt in FAMILIES[n][3]])
def test_gemm_family_strided_operands_and_output_windows(name, dtype, la, lb):
    _check_family(name, dtype, la, lb)


def test_gemm_lds_dma_tile_strided_operands_and_output_windows():
    """The LDS-DMA 128x128 tile is forced by a switch that is read once per process: ONE child process runs all of its cases."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **FAMILIES['glds'][1])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'glds', root], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'GLDS CASES OK' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---- d. split-K: writing C with ldc is the reduce launch's job, or the last workgroup's
@pytest.mark.parametrize('fused', ['0', '1', '2'])
@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('shape', SPLITK_SHAPES)
def test_gemm_splitk_output_windows(shape, dtype, fused):
    from guard_util import window
    from spatiotemporal_variable_separation_amd import ops
    M, N, K = shape
    p = _problem(M, N, K, dtype)
    out16 = dtype if dtype != F32 else BF16
    with _Env(dict(VS_GEMM_SPLITK_FUSED=fused)):
        for la, lb in LAYOUTS:
            a, b = _form(p['a'], la), _form(p['b'], lb)
            plan = _plan(dtype, M, N, K, a, la, b, lb)
            assert plan[0] == REG and plan[3] > 1, (shape, dtype, la, lb, plan)
            for od in (F32, out16):
                for epi in ('plain', 'bias_relu', 'accumulate'):
                    dense, _ = _epilogue_call(ops, p, epi, a, la, b, lb, M, N, K, od)
                    for form in WINDOWS:
                        c, gc = _window(form, M, N, od)
                        _epilogue_call(ops, p, epi, a, la, b, lb, M, N, K, od, out=c)
                        case = (shape, dtype, fused, la, lb, od, epi, form)
                        gc.check()
                        err = _rel(c, _epilogue_ref(p, epi, od))
                        assert err < _tol(od, epi == 'bias_relu'), (case, err)
                        assert torch.equal(c, dense), (case, 'differs from the dense call')


# ---- e. batched: guard bytes between the problems
def _batched(lib, dtype, batch, M, N, K, a, la, b, lb, c, accumulate):
    from spatiotemporal_variable_separation_amd import _lib, ops
    ws_bytes = lib.vs_gemm_batched_workspace_bytes(batch, M, N, K)
    ws = ops._workspace(ws_bytes, a.device) if ws_bytes else None
    _lib.check(lib.vs_gemm_batched(_lib.code_of(dtype), batch, M, N, K, a.data_ptr(), a.stride(1), a.stride(0), la, b.data_ptr(), b.stride(1), b.stride(0),
                                   lb, c.data_ptr(), c.stride(1), c.stride(0), _lib.code_of(c.dtype), 1.0, int(accumulate), ws.data_ptr() if ws is not None else 0,
                                   ws.numel() if ws is not None else 0, _lib.stream_ptr()), 'vs_gemm_batched')


@pytest.mark.parametrize('forced', [False, True])
@pytest.mark.parametrize('dtype', [BF16, F32])
def test_gemm_batched_strided_problems_and_output_windows(dtype, forced):
    """batch 3 of 64 x 48 x 72 with padded batch strides; `forced`: the ring tile (the only DMA family this small problem can be given), so the
    cases with stride_a % 8 != 0 and with A one element off are seen to fall through to the register tile.  Against fp64, and bit-equal to the
    dense batched call of the same problems wherever vs_gemm_plan returns the same row for both."""
    from guard_util import embed, window
    from oracle.detdata import det_uniform
    from spatiotemporal_variable_separation_amd import _lib
    lib = _lib.load_library()
    batch, M, N, K = 3, 64, 48, 72
    a3 = ((det_uniform((batch, M, K), 41) - 0.5) * 2.0).to(dtype)
    b3 = ((det_uniform((batch, N, K), 42) - 0.5) * 2.0).to(dtype)
    prev = det_uniform((batch, M, N), 43)
    ref = torch.bmm(a3.double(), b3.double().transpose(1, 2)).cuda()
    kind = MID if forced and dtype != F32 else REG
    with _Env(dict(VS_GEMM_MID='2', VS_GEMM_BIG='0', VS_GEMM_P8='0') if forced else {}):
        for la, lb in LAYOUTS:
            fa = (a3 if la == 0 else a3.transpose(1, 2).contiguous()).cuda()
            fb = (b3 if lb == 0 else b3.transpose(1, 2).contiguous()).cuda()
            lda, ldb = fa.shape[2] + 24, fb.shape[2] + 8
            dense_plan = _plan(dtype, M, N, K, fa, la, fb, lb, batch=batch, stride_a=fa.stride(0), stride_b=fb.stride(0))
            assert dense_plan[0] == kind, (dtype, forced, la, lb, dense_plan)
            dense = {}
            for od in (F32, dtype):
                for accumulate in (False, True):
                    d = prev.to(od).cuda() if accumulate else torch.empty((batch, M, N), dtype=od, device='cuda')
                    _batched(lib, dtype, batch, M, N, K, fa, la, fb, lb, d, accumulate)
                    dense[od, accumulate] = d
            # (stride_a - rows * lda, offset of A): fits the loader / stride_a % 8 != 0 / A one element off -> the last two: the register tile
            for sa_extra, a_off in ((16, 8), (20, 8), (16, 1)):
                a, ga = embed(fa, ld=lda, offset=a_off, batch_stride=fa.shape[1] * lda + sa_extra)
                b, gb = embed(fb, ld=ldb, offset=8, batch_stride=fb.shape[1] * ldb + 8)
                assert (a.data_ptr() % 16 == 0) == (a_off == 8)
                plan = _plan(dtype, M, N, K, a, la, b, lb, batch=batch, stride_a=a.stride(0), stride_b=b.stride(0))
                assert plan[0] == (kind if (sa_extra, a_off) == (16, 8) else REG), (dtype, forced, la, lb, sa_extra, a_off, plan)
                for od in (F32, dtype):
                    for form in WINDOWS:
                        for accumulate in (False, True):
                            c, gc = _window(form, M, N, od, batch=batch)
                            want = ref
                            if accumulate:
                                c.copy_(prev.to(od))
                                want = prev.to(od).double().cuda() + ref
                            _batched(lib, dtype, batch, M, N, K, a, la, b, lb, c, accumulate)
                            case = (dtype, forced, la, lb, sa_extra, a_off, od, form, accumulate)
                            gc.check()
                            ga.check()
                            gb.check()
                            for i in range(batch):
                                err = _rel(c[i], want[i])
                                assert err < _tol(od, False), (case, i, err)
                            if plan == dense_plan:
                                assert torch.equal(c, dense[od, accumulate]), (case, 'differs from the dense batched call')


if __name__ == '__main__':                                              # the child process of the LDS-DMA tile's test
    sys.path[:0] = [sys.argv[2], os.path.join(sys.argv[2], 'tests')]
    assert sys.argv[1] == 'glds'
    for dt in FAMILIES['glds'][3]:
        for la_, lb_ in LAYOUTS:
            _check_family('glds', dt, la_, lb_)
    print('GLDS CASES OK')

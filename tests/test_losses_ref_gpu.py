"""The fused loss kernels (vs_train_losses_fwd / _bwd / _fwd_grad, vs_frames_sse_*, vs_code_losses_*, vs_cat_bcast_bwd) against the fp64
references of tests/loss_refs.py (torch assembly of train.py:117-149, gradients by autograd) on the same fp32 / 16-bit inputs cast to
double -- never against another launch.  Shapes are the smallest that reach each path of the kernels (scalar tail, short and 4-deep vector
loops, misaligned rows, G == 1, more rows than workgroups, more code elements than one workgroup pass / one 4096-element chunk).

Bounds: scalars relative 2e-6 (the fp32 bar of test_gemm_gpu.py; a dropped row or tail element moves a sum by >= 1e-4.  Measured on an
MI355X: the fixed-order sums of vs_train_losses_fwd_grad / vs_code_losses_fwd stay below 1.9e-7, the float-atomic sums of
vs_train_losses_fwd / vs_frames_sse_fwd vary from launch to launch and reach 9e-7 at B G > 1024); fp32 gradient elements |got - ref| <= 8 * 2^-24 * |k (y - t)| (five roundings of
(k d) act'(y) with |act'| <= 1, the roundings of k and d; holds where 1 - y^2 cancels); 16-bit gradients add one rounding of the stored
type (2^-8 |ref| bf16, 2^-11 |ref| fp16, 2^-24 absolute below fp16's normal range); copies and sign flips are bit-exact.  The worst
observed errors are printed per group when the module ends (run with -s)."""
import functools

import pytest
import torch

import loss_refs as LR
from oracle.detdata import det_uniform

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
LAM = (10.0, 45.0, 0.001, 45.0)                      # (ae, s, t, pred)
UP = 0.75                                            # upstream gradient
CS = 37                                              # spatial code width: B * CS runs from 74 (one partial pass) to 25 900 elements
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
SHAPES = [(2, 3, 5, 3), (5, 1, 3, 515), (6, 6, 9, 516), (3, 4, 6, 8200), (3, 4, 6, 8201), (300, 4, 6, 36), (700, 6, 8, 8)]
T0_COLS = (19, 300)
# frames inside each activation's output range (lo, hi)
ACT_RANGE = {'none': (-1.0, 1.0), 'relu': (0.0, 2.0), 'leaky_relu': (-1.0, 1.0), 'sigmoid': (0.0, 1.0), 'tanh': (-1.0, 1.0), 'elu': (-0.9, 2.0)}
WORST = {}
ATOMIC = 'scalar (float-atomic sums): relative error'      # vs_train_losses_fwd, vs_frames_sse_fwd: the order of the partial sums varies


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
    yield
    for k in sorted(WORST):
        print('\nworst %-34s %.4g' % (k, WORST[k]))


def _note(group, value):
    WORST[group] = max(WORST.get(group, 0.0), float(value))


def _ids(v):
    return 'x'.join(str(i) for i in v) if isinstance(v, tuple) else None


# ---------------------------------------------------------------------------------------------------------------- comparisons
def check_scalars(got, ref, what, group='scalar (fixed-order sums): relative error'):
    got, ref = got.detach().cpu().double(), ref.double()
    err = (got - ref).abs()
    rel = torch.where(ref != 0, err / ref.abs().clamp_min(1e-300), err)
    print('%s: worst relative error %.3g' % (what, float(rel.max())))
    _note(group, rel.max())
    assert bool((err <= 2e-6 * ref.abs()).all()), (what, got.tolist(), ref.tolist())


def check_grad(got, ref, kd, what):
    """|got - ref| <= 8 * 2^-24 |kd| per element (+ one rounding of a 16-bit type); kd: the fp64 pre-derivative product k (y - t)."""
    dtype = got.dtype
    got = got.detach().cpu().double().reshape(ref.shape)
    bound = 8 * U24 * kd.abs()
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * ref.abs()
    elif dtype == torch.float16:
        bound = bound + 2.0 ** -11 * ref.abs() + (ref.abs() < 2.0 ** -14).double() * U24
    err = (got - ref).abs()
    frac = torch.where(bound > 0, err / bound.clamp_min(1e-300), (err > 0).double() * 1e30)
    worst = int(frac.argmax())
    name = {torch.float32: 'fp32 gradient', torch.bfloat16: 'bf16 gradient', torch.float16: 'fp16 gradient'}[dtype]
    _note(name + ': fraction of the bound', frac.flatten()[worst])
    if dtype == torch.float32:
        nz = kd != 0
        if bool(nz.any()):
            _note('fp32 gradient: error / (2^-24 |k d|)', (err[nz] / (U24 * kd[nz].abs())).max())
    assert bool((err <= bound).all()), '%s: element %d got %r ref %r bound %.3e (%.2f of it)' % (
        what, worst, got.flatten()[worst].item(), ref.flatten()[worst].item(), bound.flatten()[worst].item(), frac.flatten()[worst].item())


# ---------------------------------------------------------------------------------------------------------------- inputs
def _uniform(shape, salt, lo, hi):
    return det_uniform(shape, salt) * (hi - lo) + lo


@functools.lru_cache(maxsize=None)
def _inputs(shape, ct, act):
    """fp32 inputs on the CPU and the device.  For relu / leaky_relu the values 0.0, -0.0 and one fp32 denormal sit in the first row."""
    B, G, T, D = shape
    lo, hi = ACT_RANGE[act]
    frames = _uniform((B, G, D), 3, lo, hi)
    if act in ('relu', 'leaky_relu'):
        frames[0, 0, :3] = torch.tensor([0.0, -0.0, 1e-40])
        assert frames[0, 0, 2].item() > 0 and frames[0, 0, 2].item() < 2.0 ** -126
    cpu = dict(frames=frames, full=_uniform((B, T, D), 5, -0.25, 1.25), s_old=_uniform((B, CS), 7, -0.5, 0.5), s_new=_uniform((B, CS), 9, -0.5, 0.5),
               t0=_uniform((B, ct), 11, -0.5, 0.5))
    return cpu, {k: v.cuda() for k, v in cpu.items()}


def _targets(shape):
    """[(what the reference sees: G indices, what the kernel is given)]: an index vector with an out-of-order and a repeated target, and the
    device window (frame 0 <-> t - ae_shift, frame g <-> first_forecast + g - 1) at the first and the last legal t; the last forecast
    lands on the last observed frame."""
    B, G, T, D = shape
    idx = [(T - 1 - 2 * g) % T for g in range(G)]
    if G > 2:
        idx[-1] = idx[1]
    shift, ff = 1, T - (G - 1)
    out = [(tuple(idx), torch.tensor(idx, dtype=torch.int32).cuda())]
    for t in (shift, T - 1 + shift):
        ref_idx = LR.window_indices(t, shift, ff, G)
        assert all(0 <= i < T for i in ref_idx)
        out.append((tuple(ref_idx), (torch.tensor([t], dtype=torch.int32).cuda(), shift, ff)))
    return out


@functools.lru_cache(maxsize=None)
def _ref(shape, ct, act, idx, average, lam=LAM, with_s=True):
    cpu, _ = _inputs(shape, ct, act)
    r = LR.mlp_reference(cpu['frames'], cpu['full'], idx, cpu['s_old'] if with_s else None, cpu['s_new'] if with_s else None, cpu['t0'], lam,
                         average, UP)
    fr, fu, t0 = LR.f64(cpu['frames']), LR.f64(cpu['full']), LR.f64(cpu['t0'])
    s0, s1 = LR.frames_sse(fr, fu, idx)
    ss = (LR.f64(cpu['s_old']) - LR.f64(cpu['s_new'])).pow(2).sum() if with_s else torch.zeros((), dtype=torch.float64)
    r['raw'] = torch.stack([s0, s1, ss, t0.pow(2).sum()])
    return r


def _check_code_grads(ds_old, ds_new, dt0, ref, what):
    if ref['ds_old'] is None:
        assert ds_old is None and ds_new is None
    else:
        check_grad(ds_old, ref['ds_old'], ref['ds_old'], what + ' ds_old')
        check_grad(ds_new, ref['ds_new'], ref['ds_new'], what + ' ds_new')
        assert torch.equal(ds_new, -ds_old), what + ': ds_new is the sign flip of ds_old'
    check_grad(dt0, ref['dt0'], ref['dt0'], what + ' dt0')


# ---------------------------------------------------------------------------------------------------------------- MLP family
@pytest.mark.parametrize('ct', T0_COLS)
@pytest.mark.parametrize('average', [False, True])
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_train_losses_fwd_and_plain_bwd_match_fp64(shape, average, ct):
    from spatiotemporal_variable_separation_amd import ops
    _, d = _inputs(shape, ct, 'none')
    gt = torch.tensor(UP).cuda()
    for idx, given in _targets(shape):
        ref = _ref(shape, ct, 'none', idx, average)
        out = ops.train_losses_fwd(d['frames'], d['full'], given, d['s_old'], d['s_new'], d['t0'], LAM, average)
        dframes, ds_old, ds_new, dt0 = ops.train_losses_bwd(d['frames'], d['full'], given, d['s_old'], d['s_new'], d['t0'], LAM, average, gt)
        torch.cuda.synchronize()
        what = 'train_losses %s idx %s' % (shape, idx)
        check_scalars(out[4:9], ref['scalars'], what + ' fwd', ATOMIC)
        assert dframes.dtype == torch.float32
        check_grad(dframes, ref['dframes'], ref['dframes'], what + ' dframes')
        _check_code_grads(ds_old, ds_new, dt0, ref, what)


@pytest.mark.parametrize('act', LR.ACTS)
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_train_losses_dz_forms_match_fp64(shape, act):
    """train_losses_bwd (dz form) and train_losses_fwd_grad: dz = dL/dframes * act'(frames) in fp32 / bf16 / fp16, the code gradients, and for
    fwd_grad the four raw sums and five scalars.  D % 4 != 0 is refused (VS_ERR_ARG) by both entries."""
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd._lib import VarsepHipError
    gt = torch.tensor(UP).cuda()
    if shape[3] % 4:
        _, d = _inputs(shape, T0_COLS[0], act)
        for dt in DTYPES:
            for _, given in _targets(shape)[:2]:
                with pytest.raises(VarsepHipError, match=r'vs_train_losses_bwd failed \(-1\)'):
                    ops.train_losses_bwd(d['frames'], d['full'], given, d['s_old'], d['s_new'], d['t0'], LAM, False, gt, frames_act=act, dz_dtype=dt)
                with pytest.raises(VarsepHipError, match=r'vs_train_losses_fwd_grad failed \(-1\)'):
                    ops.train_losses_fwd_grad(d['frames'], d['full'], given, d['s_old'], d['s_new'], d['t0'], LAM, False, gt, act, dt)
        return
    seen = set()
    for ia, average in enumerate((False, True)):
        for ic, ct in enumerate(T0_COLS):
            _, d = _inputs(shape, ct, act)
            for it, (idx, given) in enumerate(_targets(shape)):
                dt = DTYPES[(ia + ic + it) % 3]                  # every (target form, dz dtype) pair occurs
                seen.add((it, dt))
                ref = _ref(shape, ct, act, idx, average)
                dz_ref = LR.dz_from(ref['dframes'], ref['frames'], act)
                args = (d['frames'], d['full'], given, d['s_old'], d['s_new'], d['t0'], LAM, average, gt)
                b_dz, b_so, b_sn, b_t0 = ops.train_losses_bwd(*args, frames_act=act, dz_dtype=dt)
                out, f_dz, f_so, f_sn, f_t0 = ops.train_losses_fwd_grad(*args, act, dt)
                torch.cuda.synchronize()
                what = 'dz %s %s %s idx %s' % (shape, act, dt, idx)
                assert b_dz.dtype == dt and f_dz.dtype == dt
                check_grad(b_dz, dz_ref, ref['dframes'], what + ' bwd dz')
                _check_code_grads(b_so, b_sn, b_t0, ref, what + ' bwd')
                check_grad(f_dz, dz_ref, ref['dframes'], what + ' fwd_grad dz')
                _check_code_grads(f_so, f_sn, f_t0, ref, what + ' fwd_grad')
                check_scalars(out[0:4], ref['raw'], what + ' fwd_grad raw sums')
                check_scalars(out[4:9], ref['scalars'], what + ' fwd_grad')
                assert torch.equal(f_dz, b_dz), what + ': fwd_grad and bwd share one formula'
    assert len(seen) == 9


def test_train_losses_without_spatial_term_match_fp64():
    """l_s = 0 and no spatial codes (n_s == 0): the term and its gradients are absent in every entry."""
    from spatiotemporal_variable_separation_amd import ops
    shape, ct, lam = (6, 6, 9, 516), 19, (10.0, 0.0, 0.001, 45.0)
    gt = torch.tensor(UP).cuda()
    for act, dt in (('none', torch.float32), ('sigmoid', torch.bfloat16), ('tanh', torch.float16)):
        _, d = _inputs(shape, ct, act)
        for idx, given in _targets(shape):
            ref = _ref(shape, ct, act, idx, False, lam, False)
            assert ref['scalars'][2].item() == 0.0
            args = (d['frames'], d['full'], given, None, None, d['t0'], lam, False)
            what = 'no spatial term %s idx %s' % (act, idx)
            out = ops.train_losses_fwd(*args)
            dframes, so, sn, dt0 = ops.train_losses_bwd(*args, gt)
            b_dz, b_so, b_sn, b_t0 = ops.train_losses_bwd(*args, gt, frames_act=act, dz_dtype=dt)
            fout, f_dz, f_so, f_sn, f_t0 = ops.train_losses_fwd_grad(*args, gt, act, dt)
            torch.cuda.synchronize()
            check_scalars(out[4:9], ref['scalars'], what + ' fwd', ATOMIC)
            check_scalars(fout[0:4], ref['raw'], what + ' fwd_grad raw sums')
            check_scalars(fout[4:9], ref['scalars'], what + ' fwd_grad')
            check_grad(dframes, ref['dframes'], ref['dframes'], what + ' dframes')
            dz_ref = LR.dz_from(ref['dframes'], ref['frames'], act)
            check_grad(b_dz, dz_ref, ref['dframes'], what + ' bwd dz')
            check_grad(f_dz, dz_ref, ref['dframes'], what + ' fwd_grad dz')
            assert torch.equal(f_dz, b_dz)
            for a, b, c in ((so, sn, dt0), (b_so, b_sn, b_t0), (f_so, f_sn, f_t0)):
                _check_code_grads(a, b, c, ref, what)


# ---------------------------------------------------------------------------------------------------------------- conv family
@pytest.mark.parametrize('shape', [(2, 3, 5, 3), (5, 1, 3, 515), (3, 4, 6, 4100), (300, 4, 6, 36)], ids=_ids)
def test_frames_sse_fwd_bwd_match_fp64(shape):
    from spatiotemporal_variable_separation_amd import ops
    B, G, T, D = shape
    cpu, d = _inputs(shape, T0_COLS[0], 'none')
    idx, idx_dev = _targets(shape)[0]                              # a repeated and an out-of-order target (G == 1: the one frame)
    fr, fu = LR.f64(cpu['frames']), LR.f64(cpu['full'])
    sums = ops.frames_sse_fwd(d['frames'], d['full'], idx_dev)
    coef = torch.tensor([0.0123, -0.0456], dtype=torch.float32)
    got = ops.frames_sse_bwd(d['frames'], d['full'], idx_dev, coef.cuda())
    torch.cuda.synchronize()
    check_scalars(sums, torch.stack(LR.frames_sse(fr, fu, idx)), 'frames_sse %s' % (shape,), ATOMIC)
    k = coef.double()[[0] + [1] * (G - 1)].view(1, G, 1)
    ref = k * (fr - fu[:, list(idx)])
    check_grad(got, ref, ref, 'frames_sse_bwd %s' % (shape,))


_F, _B, _H = torch.float32, torch.bfloat16, torch.float16
CODE_CASES = [([8], [_F]), ([8], [_B]), ([4096], [_H]), ([4096], [_F]), ([4104], [_B]), ([4104], [_H]), ([12296, 8, 4096], [_F, _B, _H]),
              ([12296, 8, 4096], [_B, _H, _F]), ([8, 16, 4096, 24, 4104, 8, 8200, 40, 8, 4096], [_F, _B, _H] * 3 + [_B]), ([], [])]
NEED = [(True, True), (True, False), (False, True), (False, False)]


@functools.lru_cache(maxsize=None)
def _conv_frames():
    B, G, T, D = 2, 3, 5, 12
    cpu = dict(recon=_uniform((B, 1, D), 21, 0.0, 1.0), fore=_uniform((B, G, D), 23, 0.0, 1.0), full=_uniform((B, T, D), 25, 0.0, 1.0))
    return cpu, {k: v.cuda() for k, v in cpu.items()}, [3], [2, 4, 2]


@pytest.mark.parametrize('t_shape', [(1, 19), (16, 256), (17, 241)], ids=_ids)
@pytest.mark.parametrize('case', range(len(CODE_CASES)))
def test_code_losses_fwd_bwd_match_fp64(case, t_shape):
    """vs_code_losses_fwd / _bwd through ops: one to ten (a, b) pairs of mixed types and sizes around the 4096-element chunk, no pair at all,
    t0 of 19 / 4096 / 4097 elements, gradients left out by the `need` flags.  The frame sums come from vs_frames_sse_fwd (as in
    functional.conv_losses); the reference is the fp64 assembly over the concatenated pairs, gradients by autograd."""
    from spatiotemporal_variable_separation_amd import ops
    counts, dtypes = CODE_CASES[case]
    lam = (1.7, 45.0, 0.01, 30.0)
    fcpu, fdev, ae_idx, f_idx = _conv_frames()
    pairs_cpu = [((_uniform((n,), 31 + 2 * j, -1.0, 1.0)).to(dt), (_uniform((n,), 32 + 2 * j, -1.0, 1.0)).to(dt)) for j, (n, dt) in enumerate(zip(counts, dtypes))]
    pairs = [(a.cuda(), b.cuda()) for a, b in pairs_cpu]
    need = [NEED[(j + case) % 4] for j in range(len(pairs))]
    t0 = _uniform(t_shape, 13, -0.5, 0.5)
    t0_dev = t0.cuda()
    assert ops.code_losses_supported(pairs, t0_dev)
    ae_dev = torch.tensor(ae_idx, dtype=torch.int32).cuda()
    f_dev = torch.tensor(f_idx, dtype=torch.int32).cuda()
    g = torch.tensor([UP]).cuda()
    scale_ae, scale_pred = 1.0 / fcpu['recon'].numel(), 1.0 / fcpu['fore'].numel()
    for average in (False, True):
        inv_t = 1.0 / t0.numel() if average else float(t0.shape[1]) / t0.numel()
        sse_ae = ops.frames_sse_fwd(fdev['recon'], fdev['full'], ae_dev)
        sse_pred = ops.frames_sse_fwd(fdev['fore'], fdev['full'], f_dev)
        out = ops.code_losses_fwd(pairs, t0_dev, sse_ae, sse_pred, scale_ae, scale_pred, lam, inv_t)
        da, db, dt0, coefs = ops.code_losses_bwd(pairs, need, t0_dev, g, scale_ae, scale_pred, lam, inv_t)
        torch.cuda.synchronize()

        recon, fore, t64 = (LR.f64(x).requires_grad_(True) for x in (fcpu['recon'], fcpu['fore'], t0))
        full = LR.f64(fcpu['full'])
        p64 = [(LR.f64(a).requires_grad_(True), LR.f64(b).requires_grad_(True)) for a, b in pairs_cpu]
        terms = LR.conv_losses(recon, fore, full, ae_idx, f_idx, p64, t64, lam, average)
        leaves = [recon, fore, t64] + [x for p in p64 for x in p]
        gr = LR.grads(terms['total'], UP, leaves)
        what = 'code_losses case %d t0 %s average %s' % (case, t_shape, average)
        check_scalars(out, torch.stack([terms[k].detach() for k in ('total', 'ae', 'zero', 'pred', 't_reg')]), what)
        # the coefficient of (y - t) in the autograd frame gradients
        d_ae, d_pred = (recon - full[:, ae_idx]).detach(), (fore - full[:, f_idx]).detach()
        c_ref = torch.stack([(gr[0] * d_ae).sum() / d_ae.pow(2).sum(), (gr[1] * d_pred).sum() / d_pred.pow(2).sum()])[[0, 0, 1, 1]]
        check_grad(coefs, c_ref, c_ref, what + ' coefs')
        assert coefs[0].item() == coefs[1].item() and coefs[2].item() == coefs[3].item()
        check_grad(dt0, gr[2], gr[2], what + ' dt0')
        assert len(da) == len(db) == len(pairs)
        for j, (a, b) in enumerate(pairs):
            ra, rb = gr[3 + 2 * j], gr[4 + 2 * j]
            for got, ref, wanted, name in ((da[j], ra, need[j][0], 'da'), (db[j], rb, need[j][1], 'db')):
                if not wanted:
                    assert got is None
                    continue
                assert got.dtype == a.dtype and got.shape == a.shape
                check_grad(got, ref, ref, '%s %s[%d]' % (what, name, j))
            if need[j][0] and need[j][1]:
                assert torch.equal(db[j], -da[j]), what + ': db is the sign flip of da'


@pytest.mark.parametrize('dout_dtype,a_dtype,x_dtype', [(_F, _F, _B), (_B, _B, _F), (_H, _F, _H)])
def test_cat_bcast_bwd_with_one_gradient_left_out(dout_dtype, a_dtype, x_dtype):
    """ops.cat_bcast_bwd with need_a / need_x off: the other gradient is the one of cat([a.repeat(n, 1, 1, 1), x], 1) by autograd in fp64."""
    from spatiotemporal_variable_separation_amd import ops
    B, n, Ca, Cb, H, W = 2, 3, 3, 2, 2, 12
    dout = _uniform((n * B, Ca + Cb, H, W), 41, -1.0, 1.0).to(dout_dtype)
    a = torch.zeros((B, Ca, H, W), dtype=torch.float64, requires_grad=True)
    x = torch.zeros((n * B, Cb, H, W), dtype=torch.float64, requires_grad=True)
    ra, rx = torch.autograd.grad(torch.cat([a.repeat(n, 1, 1, 1), x], dim=1), [a, x], dout.double())
    da, none = ops.cat_bcast_bwd(dout.cuda(), B, n, Ca, a_dtype, x_dtype, need_a=True, need_x=False)
    none2, dx = ops.cat_bcast_bwd(dout.cuda(), B, n, Ca, a_dtype, x_dtype, need_a=False, need_x=True)
    torch.cuda.synchronize()
    assert none is None and none2 is None and da.dtype == a_dtype and dx.dtype == x_dtype
    assert torch.equal(dx.cpu(), rx.to(dout_dtype).to(x_dtype))        # a copy: one conversion of the stored value
    # n terms added in fp32 in frame order: (n - 1) roundings of partial sums bounded by the sum of the magnitudes, then the stored type's
    mag = dout.double()[:, :Ca].abs().view(n, B, Ca, H, W).sum(0)
    bound = (n - 1) * U24 * mag + {_F: U24, _B: 2.0 ** -8, _H: 2.0 ** -11}[a_dtype] * ra.abs()
    err = (da.cpu().double() - ra).abs()
    _note('cat_bcast da: fraction of the bound', (err / bound).max())
    assert bool((err <= bound).all())

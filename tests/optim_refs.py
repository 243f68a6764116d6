"""fp64 references, the fp32 witness and the per-element bounds for the tests of the optimizer kernels (vs_optim.hip, vs_adam_math.h).
TEST INFRASTRUCTURE ONLY, CPU only.

`adam_step_fp64` is torch.optim.Adam itself (single-tensor path, foreach=False) on double tensors with its state loaded from the arguments --
not a re-typing of the kernel's formula.  `adam_step_fp32_emulated` IS a re-typing of vs_adam_coef / vs_adam_elem in numpy float32 (one
rounding per operation, no FMA); it is only the witness that a correct fp32 implementation fits the bounds of `adam_bounds`
(tests/test_optim_refs_cpu.py) and nothing on the GPU is asserted against it.  `grad_scaler_update` is GradScaler.update()'s state machine.
`adam_launch` builds the deterministic inputs both test modules use, so that the CPU module proves the bounds attainable on exactly the
cases the GPU module runs."""
import math

import numpy as np
import torch

from oracle.detdata import det_uniform

U24 = 2.0 ** -24
EPS = 1e-8
SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 3 * 4096 + 5)
HYPER = ((4e-4, (0.9, 0.99)), (1e-3, (0.5, 0.999)), (1e-3, (0.9, 0.999)))
STEPS = (1, 2, 7, 1000)
MAGS = (1e-6, 1.0, 1e3)
SCALES = (None, 65536.0, 3000.0)
GDTYPES = (torch.float32, torch.bfloat16)
SKIPPED = (0, 2)                                     # per tensor, alternating inside one launch
BLOCK = 40                                           # length of the exact-zero and of the g == m block (tensors of >= 1023 elements)


# ---------------------------------------------------------------------------------------------------------------- references
def adam_step_fp64(p, g, m, v, t, lr, betas, eps=EPS):
    """One Adam step in double: p, g, m, v are 1-D tensors (any float type, taken as they are), t the number of steps the parameter will
    have taken after this one.  -> dict(p, m, v, den, S, upd) of fp64 tensors / floats: den = sqrt(v') / sqrt(1 - b2^t) + eps,
    S = lr / (1 - b1^t), upd = S m' / den (the three intermediates are written out by hand: the bounds need them)."""
    q = torch.nn.Parameter(p.detach().double().clone())
    q.grad = g.detach().double().clone()
    opt = torch.optim.Adam([q], lr=lr, betas=betas, eps=eps, foreach=False)
    opt.state[q] = dict(step=torch.tensor(float(t - 1)), exp_avg=m.detach().double().clone(), exp_avg_sq=v.detach().double().clone())
    opt.step()
    st = opt.state[q]
    assert float(st['step']) == float(t)
    m1, v1 = st['exp_avg'].clone(), st['exp_avg_sq'].clone()
    b1, b2 = betas
    den = v1.sqrt() / math.sqrt(1.0 - b2 ** t) + eps
    S = lr / (1.0 - b1 ** t)
    return dict(p=q.detach().clone(), m=m1, v=v1, den=den, S=S, upd=S * m1 / den)


def adam_step_fp32_emulated(p, g, m, v, t, lr, betas, eps=EPS, scale=None):
    """vs_adam_coef + vs_adam_elem in numpy float32, operation by operation (coefficients formed in double, then cast; the optional
    unscale is g * (float32(1) / scale)).  p, m, v fp32 tensors; g fp32 or bf16 (converted exactly).  -> (p', m', v') fp32 tensors."""
    f = np.float32
    b1, b2 = betas
    w1, w2, beta2 = f(1.0 - b1), f(1.0 - b2), f(b2)
    bc1 = f(1.0 - math.pow(b1, float(t)))
    bc2_sqrt = f(math.sqrt(1.0 - math.pow(b2, float(t))))
    step_size = f(lr) / bc1
    eps = f(eps)
    p, m, v = (x.detach().numpy().astype(f) for x in (p, m, v))
    g = g.detach().float().numpy().astype(f)
    assert all(x.dtype == f for x in (p, g, m, v)) and type(step_size) is f
    if scale is not None:
        g = g * (f(1) / f(scale))
    m = m + w1 * (g - m)
    v = v * beta2 + (w2 * g) * g
    denom = np.sqrt(v) / bc2_sqrt + eps
    p = p - step_size * (m / denom)
    assert all(x.dtype == f for x in (p, m, v))
    return torch.from_numpy(p), torch.from_numpy(m), torch.from_numpy(v)


def adam_bounds(P, G, M, ref, scale=None):
    """Per-element bounds of an fp32 Adam step against `ref` = adam_step_fp64(P, G, M, V, ...); P, G, M the fp64 inputs (G already divided
    by the loss scale).  u = 2^-24.
      m: 4u max(|M|, |G|): m + w1 (g - m) rounds the difference, the product and the sum, each relative to an operand and not to the result
         (g - m cancels), and w1 itself; + 4u |G| when the loss scale is no power of two (1 / scale and g * (1 / scale) round).
      v: 8u V' + 2^-149: five roundings and those of w2, beta2, every term positive (no cancellation); one ulp of the smallest denormal.
      p: 2u max(|P|, |P'|) for the final subtraction, (S / den) bound_m for the error m brings along, 16u |upd| for the roundings of
         lr, bc1, their quotient, sqrt, its quotient, + eps, m / den and the product, and half of v's relative error through the root."""
    pow2 = scale is None or math.frexp(float(scale))[0] == 0.5
    bm = 4 * U24 * torch.maximum(M.abs(), G.abs())
    if not pow2:
        bm = bm + 4 * U24 * G.abs()
    bv = 8 * U24 * ref['v'] + 2.0 ** -149
    bp = 2 * U24 * torch.maximum(P.abs(), ref['p'].abs()) + (ref['S'] / ref['den']) * bm + 16 * U24 * ref['upd'].abs()
    return dict(p=bp, m=bm, v=bv)


def bound_fractions(got_p, got_m, got_v, ref, bounds):
    """{'p' | 'm' | 'v': (worst |got - ref| / bound, its element)}; an error where the bound is 0 counts as 1e30."""
    out = {}
    for k, got in (('p', got_p), ('m', got_m), ('v', got_v)):
        err = (got.detach().cpu().double() - ref[k]).abs()
        b = bounds[k]
        frac = torch.where(b > 0, err / b.clamp_min(1e-300), (err > 0).double() * 1e30)
        i = int(frac.argmax())
        out[k] = (float(frac[i]), i)
    return out


def grad_scaler_update(state, growth, backoff, interval):
    """torch.amp.GradScaler.update() (amp_update_scale kernel) on state = [scale, found_inf, growth_tracker, skipped]: an overflow step
    backs the scale off, resets the tracker and is counted; the `interval`-th clean step in a row grows the scale -- only to a finite
    value -- and resets the tracker; found_inf is cleared.  The factors are Python floats (doubles, as torch passes them to its kernel) and
    the scale an fp32 value: each product is formed in double and rounded once to fp32."""
    scale, found_inf, tracker, skipped = (float(x) for x in state)
    f = np.float32
    with np.errstate(over='ignore'):
        if found_inf != 0.0:
            scale = float(f(scale * float(backoff)))
            tracker = 0.0
            skipped += 1.0
        else:
            tracker += 1.0
            if tracker >= float(interval):
                grown = f(scale * float(growth))
                if np.isfinite(grown):
                    scale = float(grown)
                tracker = 0.0
    return [scale, 0.0, tracker, skipped]


# (found_inf, ...) per update() call: overflow at tracker 0 and mid-interval, growth exactly at the interval, two overflows in a row
SCRIPT = (0, 0, 1, 0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0)


def scaler_cases():
    """[(start state, growth, backoff, interval, found_inf sequence)] shared with the GPU module."""
    out = []
    for interval in (1, 2, 3):
        for backoff in (0.5, 0.25):
            out.append(([65536.0, 0.0, 0.0, 0.0], 2.0, backoff, interval, SCRIPT))
    out.append(([2.0 ** 127, 0.0, 1.0, 5.0], 2.0, 0.5, 2, (0, 0, 0, 1, 0, 0)))            # growth past fp32 range: the scale stays
    out.append(([2.0 ** 126, 0.0, 0.0, 0.0], 4.0, 0.5, 1, (0, 0, 1, 0)))
    out.append(([3000.0, 0.0, 0.0, 0.0], 1.5, 0.375, 2, SCRIPT))                          # other factors (exact in fp32, as 2 and 0.5 are)
    return out


# ---------------------------------------------------------------------------------------------------------------- shared inputs
def adam_tensor(n, salt, gdtype, scale, j=0):
    """Deterministic inputs of one tensor: p, m, v fp32, g as the kernel gets it (`gdtype`, multiplied by the loss scale).  Magnitudes 1e-6,
    1 and 1e3 alternate element by element (gradient, first moment and the root of the second share theirs).  Tensors of >= 1023 elements
    carry BLOCK gradients equal to the first moment from n/4 on and BLOCK exact-zero gradients from n/2 on, the first half of those with
    m = v = 0 as well."""
    mag = torch.tensor(MAGS, dtype=torch.float64)[(torch.arange(n) + j) % len(MAGS)]
    u = [det_uniform((n,), salt * 8 + k).double() for k in range(4)]
    s = 1.0 if scale is None else float(scale)
    p = (u[0] - 0.5).float()
    g = ((u[1] - 0.5) * 2 * mag * s).float().to(gdtype)
    m = ((u[2] - 0.5) * mag).float()
    v = ((0.05 + u[3]) * mag).pow(2).float()
    if n >= 1023:
        a = n // 4
        m[a:a + BLOCK] = (g[a:a + BLOCK].double() / s).float()        # g == m (g ~ m when 1 / scale rounds)
        z = n // 2
        g[z:z + BLOCK] = 0
        m[z:z + BLOCK // 2] = 0
        v[z:z + BLOCK // 2] = 0
    return dict(p=p, g=g, m=m, v=v)


def adam_launch(t, gdtype, scale, sizes=SIZES, salt=0):
    """The tensors of one launch: [(n, skipped_j, t_j, inputs)], and the value of the device step word.  The group has taken t + 1 steps, so
    a tensor that sat out SKIPPED[1] = 2 of them takes its t-th step and one that sat out none its (t + 2)-th: two bias corrections in
    one launch."""
    step_word = t + max(SKIPPED) - 1
    out = []
    for j, n in enumerate(sizes):
        sk = SKIPPED[(j + 1) % 2]
        out.append((n, sk, step_word + 1 - sk, adam_tensor(n, salt * 100000 + t * 64 + j, gdtype, scale, j)))
    return out, step_word


def reference_of(inp, t_j, lr, betas, scale):
    """(fp64 inputs P, G, M, V, the fp64 step, its bounds) of one tensor of adam_launch."""
    s = 1.0 if scale is None else float(scale)
    P, M, V = inp['p'].double(), inp['m'].double(), inp['v'].double()
    G = inp['g'].double() / s
    ref = adam_step_fp64(P, G, M, V, t_j, lr, betas, EPS)
    return P, G, M, V, ref, adam_bounds(P, G, M, ref, scale)


def first_step_tensor(j):
    """(p, g) of parameter j of the 130-parameter group that takes its first step (m = v = 0, t = 1) through optim.Adam."""
    n = (1, 3, 5, 17, 1025, 4, 260, 4099)[j % 8]
    return det_uniform((n,), 300 + j) - 0.5, (det_uniform((n,), 500 + j) - 0.5) * MAGS[j % 3]

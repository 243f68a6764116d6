"""fp64 references of the training losses, for the tests of the fused loss / element-wise kernels.  TEST INFRASTRUCTURE ONLY.

Plain torch on the CPU in double precision: the assembly of the reference's train.py:38-42 (zero-order loss), :85-86 (auto-encoding MSE),
:139 (forecast MSE), :141-149 (t_reg and the weighted total) written with F.mse_loss / pow / mean, NOT the kernels' `sum * 1/N` and
`2/N (y - t)` forms.  Every gradient comes from torch.autograd on that assembly.  The only hand-written derivatives are the six "derivative
from the output" rules of the activations (networks/utils.py:50-72), which the `dz` form of the kernels needs on top of dL/dframes.
Anchored against oracle/cpu_ref.py by tests/test_loss_refs_cpu.py."""
import numpy as np
import torch
import torch.nn.functional as F

ACTS = ('none', 'relu', 'leaky_relu', 'sigmoid', 'tanh', 'elu')

# nn.LeakyReLU(0.2) on fp32 tensors multiplies by the fp32 constant nearest to 0.2 (the scalar is cast to the tensor's type); the operation
# under test is the fp32 one, so the fp64 references carry THAT slope (0.2 in double differs from it by 1.5e-8 relative: invisible to the
# gradient bounds, but it moves the last bit of one fp32 product in three).
LEAKY_SLOPE = float(np.float32(0.2))

# activation(x) in fp64
ACT_FWD = {
    'none': lambda x: x.clone(),
    'relu': lambda x: torch.where(x > 0, x, torch.zeros_like(x)),
    'leaky_relu': lambda x: torch.where(x > 0, x, LEAKY_SLOPE * x),
    'sigmoid': lambda x: torch.sigmoid(x),
    'tanh': lambda x: torch.tanh(x),
    'elu': lambda x: torch.where(x > 0, x, torch.expm1(x)),
}

# d activation / d input, written in terms of the OUTPUT y (what an in-place activation's backward has: nn.ReLU(inplace=True) etc.)
ACT_GRAD_FROM_OUT = {
    'none': lambda y: torch.ones_like(y),
    'relu': lambda y: torch.where(y > 0, torch.ones_like(y), torch.zeros_like(y)),
    'leaky_relu': lambda y: torch.where(y > 0, torch.ones_like(y), torch.full_like(y, LEAKY_SLOPE)),
    'sigmoid': lambda y: y * (1 - y),
    'tanh': lambda y: 1 - y * y,
    'elu': lambda y: torch.where(y > 0, torch.ones_like(y), y + 1),
}


def f64(t):
    """The same values in double (None stays None); a fresh leaf-able tensor."""
    return None if t is None else t.detach().cpu().double().clone()


def window_indices(t, ae_shift, first_forecast, G):
    """The device-window target rule as an index list: frame 0 <-> full[:, t - ae_shift] (train.py:85), frame g >= 1 <->
    full[:, first_forecast + g - 1] (train.py:135-139)."""
    return [int(t) - int(ae_shift)] + [int(first_forecast) + g - 1 for g in range(1, G)]


def t_reg_term(t0, average_tloss):
    """train.py:145-148."""
    if average_tloss:
        return 0.5 * (t0.pow(2).view(t0.shape[0], -1)).mean()
    return 0.5 * torch.sum(t0.pow(2), dim=1).mean()


def mlp_losses(frames, full, idx, s_old, s_new, t0, lambdas, average_tloss):
    """train.py:117-149 for a decoded stack frames [B, G, D] (frame 0: the auto-encoding reconstruction, frames 1..: the forecasts) against
    full [B, T, D]; idx: G python ints, the frame of `full` each decoded frame is compared with.  lambdas = (ae, s, t, pred).
    -> dict(total, ae, zero, pred, t_reg) of 0-d double tensors (differentiable in the inputs).  Without forecasts (G == 1) and without
    spatial codes (s_old is None) the term is absent: 0."""
    l_ae, l_s, l_t, l_pred = (float(v) for v in lambdas)
    idx = [int(i) for i in idx]
    G = frames.shape[1]
    assert len(idx) == G
    ae = F.mse_loss(full[:, idx[0]], frames[:, 0], reduction='mean')
    pred = F.mse_loss(frames[:, 1:], full[:, idx[1:]]) if G > 1 else torch.zeros((), dtype=frames.dtype)
    zero = (s_old - s_new).pow(2).mean() if s_old is not None else torch.zeros((), dtype=frames.dtype)
    t_reg = t_reg_term(t0, average_tloss)
    total = 0
    total += l_ae * ae
    total += l_s * zero
    total += l_pred * pred
    total += l_t * t_reg
    return dict(total=total, ae=ae, zero=zero, pred=pred, t_reg=t_reg)


def conv_losses(recon, fore, full, ae_idx, f_idx, pairs, t0, lambdas, average_tloss):
    """The conv families' form: recon [B, 1, D] against full[:, ae_idx], fore [B, G, D] against full[:, f_idx], the zero-order loss as ONE
    mean over the concatenation of every (a, b) pair (train.py:38-42 with skip connections; no pair: the term is absent), t_reg of t0."""
    l_ae, l_s, l_t, l_pred = (float(v) for v in lambdas)
    ae = F.mse_loss(full[:, [int(i) for i in ae_idx]], recon, reduction='mean')
    pred = F.mse_loss(fore, full[:, [int(i) for i in f_idx]])
    if pairs:
        a = torch.cat([x.flatten() for x, _ in pairs])
        b = torch.cat([y.flatten() for _, y in pairs])
        zero = (a - b).pow(2).mean()
    else:
        zero = torch.zeros((), dtype=t0.dtype)
    t_reg = t_reg_term(t0, average_tloss)
    total = l_ae * ae + l_s * zero + l_pred * pred + l_t * t_reg
    return dict(total=total, ae=ae, zero=zero, pred=pred, t_reg=t_reg)


def frames_sse(frames, full, idx):
    """(sum of squared errors of frame 0, of frames 1..) of frames [B, G, D] against full[:, idx]."""
    d = (frames - full[:, [int(i) for i in idx]]).pow(2)
    return d[:, 0].sum(), d[:, 1:].sum()


def grads(total, g, leaves):
    """d (g * total) / d leaf for every leaf (None for a leaf that is None), by autograd."""
    live = [x for x in leaves if x is not None]
    got = iter(torch.autograd.grad(float(g) * total, live, allow_unused=True))
    out = []
    for x in leaves:
        if x is None:
            out.append(None)
            continue
        v = next(got)
        out.append(torch.zeros_like(x) if v is None else v)
    return out


def mlp_reference(frames, full, idx, s_old, s_new, t0, lambdas, average_tloss, g):
    """Everything the MLP-family kernels produce, in fp64, from the fp32 inputs as they are: dict(scalars [total, ae, zero, pred, t_reg],
    dframes, ds_old, ds_new, dt0)."""
    fr, fu, so, sn, t = (f64(x) for x in (frames, full, s_old, s_new, t0))
    for x in (fr, so, sn, t):
        if x is not None:
            x.requires_grad_(True)
    terms = mlp_losses(fr, fu, idx, so, sn, t, lambdas, average_tloss)
    dfr, dso, dsn, dt = grads(terms['total'], g, [fr, so, sn, t])
    scal = torch.stack([terms[k].detach() for k in ('total', 'ae', 'zero', 'pred', 't_reg')])
    return dict(scalars=scal, dframes=dfr, ds_old=dso, ds_new=dsn, dt0=dt, frames=fr.detach())


def dz_from(dframes, frames64, act):
    """Gradient of the activation's INPUT when `frames64` are its outputs: dL/dframes * act'(from the output)."""
    return dframes * ACT_GRAD_FROM_OUT[act](frames64)

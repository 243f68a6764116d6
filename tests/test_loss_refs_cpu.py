"""tests/loss_refs.py (the fp64 references of the loss-kernel tests) against the oracle's own loss assembly (oracle/cpu_ref.py:
zero_order_loss, ae_loss, training_losses = train.py:38-42, 45-88, 111-149) on one small case, values and autograd gradients: the reference
the GPU tests lean on is itself anchored."""
import pytest
import torch

import loss_refs as LR
from oracle import cpu_ref
from oracle.detdata import det_uniform


class _FixedNet:
    """A separable net whose parts return prepared tensors: the oracle's loss code runs unchanged, the networks are taken out."""

    def __init__(self, s_old, s_new, recon, forecasts, t_codes):
        self.s = [s_old, s_new]                      # ae_loss encodes the first window, then the last one
        self.recon, self.forecasts, self.t_codes = recon, forecasts, t_codes

    def Es(self, x, return_skip=False):
        return self.s.pop(0)

    def Et(self, x):
        return None

    def decoder(self, s, t, skip=None):
        return self.recon

    def get_forecast(self, cond, n, init_s_code=None):
        return self.forecasts, self.t_codes, None, None


def _u(shape, salt, lo=-1.0, hi=1.0):
    return (det_uniform(shape, salt).double() * (hi - lo) + lo).requires_grad_(True)


@pytest.mark.parametrize('average', [False, True])
@pytest.mark.parametrize('offset', [0, 3])
def test_mlp_reference_equals_oracle_training_losses(average, offset):
    B, D, nt_cond, nt_pred, Ct = 3, 7, 3, 4, 5
    T = nt_cond + nt_pred
    n = nt_pred + offset
    cond, target = _u((B, nt_cond, D), 1).detach(), _u((B, nt_pred, D), 2).detach()
    full = torch.cat([cond, target], dim=1)
    lam = (10.0, 45.0, 0.001, 45.0)                  # (ae, s, t, pred)
    t_random = 5

    def leaves():
        return _u((B, 6), 3), _u((B, 6), 4), _u((B, D), 5), _u((B, n, D), 6), _u((B, n, Ct), 7)
    s_old, s_new, recon, fore, t_codes = leaves()
    total, terms, _, _ = cpu_ref.training_losses(cond, target, _FixedNet(s_old, s_new, recon, fore, t_codes), nt_cond, nt_pred, offset, False,
                                                 lam[0], lam[1], lam[2], lam[3], average_tloss=average, t_random=t_random)
    want = torch.autograd.grad(0.75 * total, [s_old, s_new, recon, fore, t_codes])

    s_old2, s_new2, recon2, fore2, t_codes2 = leaves()
    frames = torch.cat([recon2.unsqueeze(1), fore2], dim=1)
    idx = LR.window_indices(t_random, offset, nt_cond if offset == 0 else 0, 1 + n)
    assert idx[0] == t_random - offset and idx[1:] == list(range(T - n, T))
    got = LR.mlp_losses(frames, full, idx, s_old2, s_new2, t_codes2[:, 0], lam, average)
    assert got['total'].item() == pytest.approx(total.item(), rel=1e-14)
    for k in ('ae', 'zero', 'pred', 't_reg'):
        assert got[k].item() == pytest.approx(terms[k].item(), rel=1e-14), k
    grads = LR.grads(got['total'], 0.75, [s_old2, s_new2, recon2, fore2, t_codes2])
    for a, b in zip(grads, want):
        torch.testing.assert_close(a, b, rtol=1e-13, atol=1e-18)

    # the packaged form the GPU tests call: same numbers from the fp32 inputs cast to double, dz = dframes * act'(y)
    ref = LR.mlp_reference(frames.detach().float(), full.float(), idx, None, None, t_codes2[:, 0].detach().float(), lam, average, 0.75)
    assert ref['scalars'][2].item() == 0.0 and ref['ds_old'] is None
    y = ref['frames']
    for act in LR.ACTS:
        x = y.clone().requires_grad_(True)           # derivative from the output == autograd through the activation, where y = act(x)
        out = LR.ACT_FWD[act](x)
        (auto,) = torch.autograd.grad(out, x, torch.ones_like(out))
        torch.testing.assert_close(LR.ACT_GRAD_FROM_OUT[act](out.detach()), auto, rtol=1e-13, atol=0)
        assert torch.equal(LR.dz_from(ref['dframes'], y, act), ref['dframes'] * LR.ACT_GRAD_FROM_OUT[act](y))
    x = torch.tensor([-3.0, -0.0, 0.0, 2.5], dtype=torch.float64)
    torch.testing.assert_close(LR.ACT_FWD['elu'](x), torch.nn.functional.elu(x), rtol=1e-15, atol=0)
    torch.testing.assert_close(LR.ACT_FWD['leaky_relu'](x), torch.nn.functional.leaky_relu(x, 0.2), rtol=1e-7, atol=0)
    assert LR.ACT_FWD['leaky_relu'](x.float()).dtype == torch.float32
    assert torch.equal(LR.ACT_FWD['leaky_relu'](x).float(), torch.nn.functional.leaky_relu(x.float(), 0.2))   # the fp32 module's slope


def test_conv_reference_equals_oracle_zero_order_loss_with_skips():
    B = 2
    a = (_u((B, 8), 11), [_u((B, 2, 4, 4), 12), _u((B, 3, 2, 2), 13)])
    b = (_u((B, 8), 14), [_u((B, 2, 4, 4), 15), _u((B, 3, 2, 2), 16)])
    want = cpu_ref.zero_order_loss(a, b, True)
    pairs = [(a[0], b[0])] + list(zip(a[1], b[1]))
    full = _u((B, 5, 6), 17).detach()
    recon, fore, t0 = _u((B, 1, 6), 18), _u((B, 2, 6), 19), _u((B, 3, 2, 2), 20)
    lam = (1.7, 45.0, 0.01, 30.0)
    for average in (False, True):
        got = LR.conv_losses(recon, fore, full, [4], [1, 2], pairs, t0, lam, average)
        assert got['zero'].item() == pytest.approx(want.item(), rel=1e-14)
        ae = torch.nn.functional.mse_loss(full[:, 4], recon[:, 0])
        pred = torch.nn.functional.mse_loss(fore, full[:, 1:3])
        treg = 0.5 * t0.pow(2).view(B, -1).mean() if average else 0.5 * torch.sum(t0.pow(2), dim=1).mean()
        assert got['total'].item() == pytest.approx((lam[0] * ae + lam[1] * want + lam[3] * pred + lam[2] * treg).item(), rel=1e-14)
        s0, s1 = LR.frames_sse(fore, full, [1, 2])
        assert ((s0 + s1) / fore.numel()).item() == pytest.approx(pred.item(), rel=1e-14)
    assert LR.conv_losses(recon, fore, full, [4], [1, 2], [], t0, lam, False)['zero'].item() == 0.0

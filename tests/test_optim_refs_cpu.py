"""tests/optim_refs.py (the fp64 references and bounds of the optimizer-kernel tests) anchored on the CPU: the state-loading wrapper equals a
plain torch.optim.Adam run in double, the GradScaler state machine equals torch's own CPU kernel, and -- the condition that keeps the GPU
module from being impossible or vacuous -- a correct fp32 implementation (the operation-by-operation numpy emulation of vs_adam_elem) uses
at most 0.75 of every bound on every (hyper-parameters, t, magnitude, scale, gradient dtype) combination the GPU module runs."""
import pytest
import torch

import optim_refs as OR
from oracle.detdata import det_uniform


def _sid(s):
    return 'noscale' if s is None else 'scale%d' % s


@pytest.mark.parametrize('scale', OR.SCALES, ids=_sid)
@pytest.mark.parametrize('gdtype', OR.GDTYPES, ids=['g32', 'gbf16'])
@pytest.mark.parametrize('t', OR.STEPS)
def test_fp32_emulation_uses_at_most_three_quarters_of_every_bound(t, gdtype, scale):
    worst = {'p': 0.0, 'm': 0.0, 'v': 0.0}
    for lr, betas in OR.HYPER:
        tensors, _ = OR.adam_launch(t, gdtype, scale)
        assert {tj for _, _, tj, _ in tensors} == {t, t + 2} and {n for n, _, _, _ in tensors} == set(OR.SIZES)
        for n, sk, tj, inp in tensors:
            P, G, M, V, ref, bounds = OR.reference_of(inp, tj, lr, betas, scale)
            p, m, v = OR.adam_step_fp32_emulated(inp['p'], inp['g'], inp['m'], inp['v'], tj, lr, betas, OR.EPS, scale)
            for k, (frac, i) in OR.bound_fractions(p, m, v, ref, bounds).items():
                worst[k] = max(worst[k], frac)
                assert frac <= 0.75, (k, n, tj, lr, betas, i, frac)
            if n >= 1023:
                z = n // 2                                    # g = m = v = 0: nothing moves
                assert torch.equal(p[z:z + OR.BLOCK // 2], inp['p'][z:z + OR.BLOCK // 2])
                assert not bool(m[z:z + OR.BLOCK // 2].any()) and not bool(v[z:z + OR.BLOCK // 2].any())
    print('emulation / bound, t %d %s %s: p %.3f m %.3f v %.3f' % (t, gdtype, _sid(scale), worst['p'], worst['m'], worst['v']))
    assert min(worst.values()) > 0.05                          # and the bounds are not orders of magnitude loose


def test_fp32_emulation_of_a_first_step_fits_the_bounds():
    """The 130 parameters the GPU module sends through optim.Adam (m = v = 0, t = 1)."""
    lr, betas = OR.HYPER[0]
    for j in range(130):
        p, g = OR.first_step_tensor(j)
        z = torch.zeros_like(p)
        ref = OR.adam_step_fp64(p, g, z, z, 1, lr, betas, OR.EPS)
        bounds = OR.adam_bounds(p.double(), g.double(), z.double(), ref)
        for k, (frac, i) in OR.bound_fractions(*OR.adam_step_fp32_emulated(p, g, z, z, 1, lr, betas), ref, bounds).items():
            assert frac <= 0.75, (j, k, i, frac)


def test_bounds_catch_the_errors_the_gpu_module_is_there_for():
    """A wrong bias correction (t off by two), a gradient left scaled and a learning rate off by 1e-4 relative all leave the bounds."""
    for t, (lr, betas) in ((1, OR.HYPER[0]), (7, OR.HYPER[0]), (1000, OR.HYPER[2])):      # 0.99^1000 is below fp32 resolution of 1, 0.999^1000 not
        n, inp = 4097, OR.adam_tensor(4097, 5, torch.float32, 3000.0)
        P, G, M, V, ref, bounds = OR.reference_of(inp, t, lr, betas, 3000.0)
        args = (inp['p'], inp['g'], inp['m'], inp['v'])
        wrong_t = OR.adam_step_fp32_emulated(*args, t + 2, lr, betas, OR.EPS, 3000.0)
        unscaled = OR.adam_step_fp32_emulated(*args, t, lr, betas, OR.EPS, None)
        wrong_lr = OR.adam_step_fp32_emulated(*args, t, lr * 1.0001, betas, OR.EPS, 3000.0)
        assert OR.bound_fractions(*wrong_t, ref, bounds)['p'][0] > 1.0
        assert OR.bound_fractions(*unscaled, ref, bounds)['m'][0] > 1.0 and OR.bound_fractions(*unscaled, ref, bounds)['v'][0] > 1.0
        assert OR.bound_fractions(*wrong_lr, ref, bounds)['p'][0] > 1.0


def test_adam_step_fp64_equals_a_plain_fp64_adam_run():
    """Five steps of torch.optim.Adam in double against five single steps of adam_step_fp64 chained through its returned state, to 1e-14
    relative; the second parameter has grad=None at the third step, so its own step count falls one behind."""
    lr, betas = 1e-3, (0.9, 0.999)
    shapes = [(37,), (5,)]
    ps = [torch.nn.Parameter(det_uniform(s, 50 + i).double() - 0.5) for i, s in enumerate(shapes)]
    opt = torch.optim.Adam(ps, lr=lr, betas=betas, eps=OR.EPS, foreach=False)
    mine = [dict(p=p.detach().clone(), m=torch.zeros_like(p), v=torch.zeros_like(p), t=0) for p in ps]
    for step in range(5):
        for i, (p, st) in enumerate(zip(ps, mine)):
            if step == 2 and i == 1:
                p.grad = None
                continue
            g = (det_uniform(p.shape, 60 + 10 * step + i).double() - 0.5) * 10.0 ** (step - 2)
            p.grad = g.clone()
            st['t'] += 1
            r = OR.adam_step_fp64(st['p'], g, st['m'], st['v'], st['t'], lr, betas, OR.EPS)
            st.update(p=r['p'], m=r['m'], v=r['v'])
        opt.step()
        for p, st in zip(ps, mine):
            torch.testing.assert_close(st['p'], p.detach(), rtol=1e-14, atol=0)
            torch.testing.assert_close(st['m'], opt.state[p]['exp_avg'], rtol=1e-14, atol=0)
            torch.testing.assert_close(st['v'], opt.state[p]['exp_avg_sq'], rtol=1e-14, atol=0)
            assert float(opt.state[p]['step']) == st['t']
    assert [st['t'] for st in mine] == [5, 4]
    # the hand-written intermediates are those of the step: p' = p - upd
    g = det_uniform((37,), 99).double() - 0.5
    r = OR.adam_step_fp64(mine[0]['p'], g, mine[0]['m'], mine[0]['v'], 6, lr, betas, OR.EPS)
    torch.testing.assert_close(mine[0]['p'] - r['upd'], r['p'], rtol=1e-14, atol=0)


def test_grad_scaler_update_equals_torch_cpu_kernel():
    """torch._amp_update_scale_ accepts CPU tensors in the installed torch: the Python state machine follows it call by call, including the
    step where the grown scale would exceed fp32 range (torch keeps the old scale and still resets the tracker)."""
    for start, growth, backoff, interval, script in OR.scaler_cases() + [([3000.0, 0.0, 0.0, 0.0], 1.7, 0.3, 2, OR.SCRIPT)]:
        state = list(start)
        scale = torch.tensor([start[0]], dtype=torch.float32)
        tracker = torch.tensor([int(start[2])], dtype=torch.int32)
        skipped = start[3]
        for k, inf in enumerate(script):
            state[1] = float(inf)
            state = OR.grad_scaler_update(state, growth, backoff, interval)
            torch._amp_update_scale_(scale, tracker, torch.tensor([float(inf)]), growth, backoff, interval)
            skipped += inf
            assert state == [scale.item(), 0.0, float(tracker.item()), skipped], (start, growth, backoff, interval, k)
            assert state[0] != float('inf')
    assert OR.grad_scaler_update([2.0 ** 127, 0.0, 0.0, 0.0], 2.0, 0.5, 1) == [2.0 ** 127, 0.0, 0.0, 0.0]

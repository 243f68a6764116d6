"""vs_gemm_adam_paced (the weight-gradient + Adam launch as a few workgroups that walk the tiles) against vs_gemm_adam: the same update bit for
bit -- parameter, both moments, the 16-bit operand copy -- for every cap on the grid, every number of state pieces in flight and both
cache policies; nothing outside the tensors is written; a raised guard word leaves everything alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(128, 128, 32),        # one whole tile, one K tile
          (384, 264, 72),        # 3 x 3 tiles, ragged last column tile, K tail
          (136, 264, 40)]        # ragged rows (the ragged case of test_optim_gpu.py)
CAPS = [1, 2, 4, 1000]           # one workgroup walks everything; 4 does not divide 9; above the tile count
LR, BETAS, EPS = 4e-4, (0.9, 0.99), 1e-8
_REF = {}


def _operands(shape, step):
    from oracle.detdata import det_uniform
    M, N, K = shape
    dz = ((det_uniform((K, M), 10 + step) - 0.5) * 0.1).cuda().bfloat16()
    h = (det_uniform((K, N), 20 + step) - 0.5).cuda().bfloat16()
    return dz, h


def _start(shape):
    from oracle.detdata import det_uniform
    M, N, _ = shape
    return (det_uniform((M, N), 3) - 0.5).cuda()


def _reference(shape, copy):
    """[(param, exp_avg, exp_avg_sq, copy)] after each of three vs_gemm_adam steps; computed once per (shape, copy dtype) and not modified."""
    key = (shape, copy)
    if key not in _REF:
        from spatiotemporal_variable_separation_amd import ops
        M, N, K = shape
        p, m, v = _start(shape), torch.zeros(M, N, device='cuda'), torch.zeros(M, N, device='cuda')
        sh = None if copy is None else torch.zeros(M, N, device='cuda', dtype=copy)
        step = torch.zeros(1, dtype=torch.int32, device='cuda')
        out = []
        for s in range(3):
            dz, h = _operands(shape, s)
            ops.gemm_adam(dz, ops.LAYOUT_S, h, ops.LAYOUT_S, M, N, K, p, m, v, sh, step, 0, LR, BETAS, EPS)
            step += 1
            out.append(tuple(None if t is None else t.clone() for t in (p, m, v, sh)))
        torch.cuda.synchronize()
        _REF[key] = out
    return _REF[key]


def _padded(M, N, dtype, fill):
    """An [M, N] view with ldc = N + 8 at element offset 8 + ... of a larger allocation filled with `fill` (the canary)."""
    ldc = N + 8
    buf = torch.full((16 + M * ldc + 16,), fill, dtype=dtype, device='cuda')
    return buf, buf[16:16 + M * ldc].view(M, ldc)[:, :N]


def _canaries_intact(buf, view, fill):
    mask = torch.ones_like(buf, dtype=torch.bool)
    M, N = view.shape
    mask[16:16 + M * view.stride(0)].view(M, view.stride(0))[:, :N] = False
    return bool((buf[mask] == fill).all())


@pytest.mark.parametrize('policy', [0, 1])
@pytest.mark.parametrize('pieces', [1, 2, 4])
@pytest.mark.parametrize('copy', [torch.bfloat16, torch.float16, None])
@pytest.mark.parametrize('shape', SHAPES)
def test_paced_equals_gemm_adam_bitwise(shape, copy, pieces, policy):
    """Every cap, three steps each; the tensors are row-strided views (ldc = N + 8) at a non-zero offset inside allocations whose other
    words are canaries."""
    from spatiotemporal_variable_separation_amd import ops
    M, N, K = shape
    ref = _reference(shape, copy)
    for cap in CAPS:
        bufs = [_padded(M, N, torch.float32, -7.25) for _ in range(3)]
        (pb, p), (mb, m), (vb, v) = bufs
        p.copy_(_start(shape)); m.zero_(); v.zero_()
        sb, sh = (None, None) if copy is None else _padded(M, N, copy, -7.25)
        step = torch.zeros(1, dtype=torch.int32, device='cuda')
        for s in range(3):
            dz, h = _operands(shape, s)
            ops.gemm_adam_paced(dz, ops.LAYOUT_S, h, ops.LAYOUT_S, M, N, K, p, m, v, sh, step, 0, LR, BETAS, EPS, cap, pieces, policy)
            step += 1
            torch.cuda.synchronize()
            rp, rm, rv, rs = ref[s]
            assert torch.equal(p, rp), (cap, s, 'param', (p - rp).abs().max().item())
            assert torch.equal(m, rm) and torch.equal(v, rv), (cap, s, 'moments')
            if copy is not None:
                assert torch.equal(sh, rs), (cap, s, 'copy')
        for buf, view in ((pb, p), (mb, m), (vb, v)) + (() if copy is None else ((sb, sh),)):
            assert _canaries_intact(buf, view, -7.25), (cap, 'a word outside the tensor was written')


def test_paced_with_the_guard_raised_writes_nothing():
    from spatiotemporal_variable_separation_amd import ops
    dev = torch.device('cuda', torch.cuda.current_device())
    guard = ops.exchange_guard(dev)
    assert guard is not None and ops.rollout_exchange_error(dev) == 0
    shape = SHAPES[1]
    M, N, K = shape
    p, m, v = _start(shape), torch.rand(M, N, device='cuda'), torch.rand(M, N, device='cuda')
    sh = torch.full((M, N), 3.0, device='cuda', dtype=torch.bfloat16)
    before = [t.clone() for t in (p, m, v, sh)]
    step = torch.full((1,), 5, dtype=torch.int32, device='cuda')
    dz, h = _operands(shape, 0)
    try:
        guard[0] = 1
        for cap in (2, 1000):
            ops.gemm_adam_paced(dz, ops.LAYOUT_S, h, ops.LAYOUT_S, M, N, K, p, m, v, sh, step, 0, LR, BETAS, EPS, cap, 4, 0)
        torch.cuda.synchronize()
        for t, b in zip((p, m, v, sh), before):
            assert torch.equal(t, b)
        assert int(step.item()) == 5
    finally:
        assert ops.rollout_exchange_error(dev) == 1 and ops.rollout_exchange_error(dev) == 0      # reported once, cleared by the read
    ops.gemm_adam_paced(dz, ops.LAYOUT_S, h, ops.LAYOUT_S, M, N, K, p, m, v, sh, step, 0, LR, BETAS, EPS, 2, 4, 0)
    torch.cuda.synchronize()
    assert not torch.equal(p, before[0]), 'with the word cleared the same call updates'

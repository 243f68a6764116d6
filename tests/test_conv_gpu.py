"""GPU parity of the convolution / BatchNorm / pooling kernels (through the C ABI) against torch CPU fp64 ops.

fp32 compute: tolerance 1e-5 relative L2 (exact-fp32 MFMA; only the summation order differs from ATen).
bf16 compute: operands are bf16-rounded first, then compared with the fp64 result on those rounded operands
(tolerance 1e-5 on fp32 outputs): the kernel adds no error beyond the stated operand rounding.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (B, Cin, H, W, Cout, k, stride, pad, transposed)  -- every conv geometry the reference uses, at reduced widths
GEOMS = [
    (3, 5, 64, 64, 8, 4, 2, 1, False),      # DCGAN encoder layer 0 (conv.py:119)
    (2, 16, 16, 16, 32, 4, 2, 1, False),    # DCGAN encoder mid layers
    (3, 8, 32, 32, 8, 3, 1, 1, False),      # VGG / SST / ConvResBlock 3x3
    (2, 12, 4, 4, 7, 4, 1, 0, False),       # VGG encoder last_op: 4x4 valid -> 1x1
    (4, 11, 1, 1, 16, 4, 1, 0, True),       # decoder first_upconv: 1x1 -> 4x4 (conv.py:258,295)
    (2, 16, 8, 8, 8, 4, 2, 1, True),        # DCGAN decoder k4 s2 p1
    (3, 8, 32, 32, 1, 4, 2, 1, True),       # DCGAN decoder last layer (Cout = nc = 1)
    (2, 6, 16, 16, 2, 3, 1, 1, True),       # VGG decoder last layer: ConvTranspose2d k3 s1 p1
    (1, 130, 8, 8, 70, 3, 1, 1, False),     # odd channel counts (K and M tails)
    # >= 64 output channels and >= 2^20 (pixel, tap-channel) pairs: the "gather once into a column matrix + dense GEMM" path
    (16, 64, 32, 32, 64, 4, 2, 1, False),   # k4 s2 gather kernel (fwd, wgrad), stride-1 phase kernel at 16x16 (dgrad)
    (16, 64, 16, 16, 64, 4, 2, 1, True),    # phases at 16x16 (fwd), k4 s2 gather of dy + reuse by dgrad
    (32, 128, 8, 8, 64, 4, 2, 1, True),     # 8-pixel rows: every unit is a full row (no neighbours)
    (128, 128, 4, 4, 64, 4, 2, 1, True),    # 4x4 maps: generic gather kernel (two rows per 16-byte unit)
    (2, 64, 32, 32, 96, 3, 1, 1, False),    # 3x3 pad 1 (VGG / SST widths): stride-1 kernel with all nine taps
    (2, 72, 24, 24, 64, 3, 1, 1, True),     # ConvTranspose2d k3 s1 p1, flipped taps, rows of 24 pixels
    (64, 148, 1, 1, 512, 4, 1, 0, True),    # decoder first_upconv at full width: 1x1 -> 4x4 through the column matrix
    (64, 128, 4, 4, 64, 4, 1, 0, False),    # VGG encoder last_op at width: its input gradient gathers dy on the 4x4 grid
    # chairs ResNet18 encoder (conv.py:433-564): 25-tap stem, odd sizes, stride-2 3x3 and 1x1 convs whose input gradients
    # run as four parity phases of DIFFERENT extents (one of them without taps for the 1x1 kernel)
    (2, 15, 64, 64, 16, 5, 2, 3, False),    # stem: k5 s2 p3, 64 -> 33
    (3, 8, 17, 17, 12, 3, 2, 1, False),     # layer2.0.conv1: k3 s2 p1, 17 -> 9
    (3, 8, 17, 17, 12, 1, 2, 0, False),     # layer2.0.downsample.0: k1 s2 p0, 17 -> 9
    (2, 16, 9, 9, 24, 3, 2, 1, False),      # 9 -> 5
    (2, 16, 5, 5, 24, 1, 2, 0, False),      # 5 -> 3
    (4, 24, 3, 3, 10, 3, 1, 0, False),      # conv_out: 3x3 valid -> 1x1
    (4, 64, 33, 33, 64, 3, 2, 1, False),    # 33 -> 17 with 64 channels: the column-matrix path on odd sizes
    (3, 8, 32, 32, 3, 4, 2, 1, True),       # DCGAN decoder last layer for 3-channel frames (chairs): one-pass kernel with 4 row slots
    (64, 128, 4, 4, 64, 3, 1, 1, False),    # 3x3 on 4x4 maps at width (VGG encoder / decoder 512-channel layers): one-map-per-thread column gather,
    (72, 64, 4, 4, 128, 3, 1, 1, True),     #   weight gradient through the dense transposed copy of the channel-rows operand
    (64, 64, 8, 8, 128, 4, 2, 1, False),    # DCGAN encoder c4 geometry (8x8 -> 4x4): k4 s2 column gather with one 8x8 map per thread
]


def _rand(shape, salt, scale=1.0):
    from oracle.detdata import det_uniform
    return (det_uniform(shape, salt) - 0.5) * 2.0 * scale


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('geom', GEOMS)
def test_conv_fwd_dgrad_wgrad(dtype, geom):
    from spatiotemporal_variable_separation_amd import ops
    B, Cin, H, W, Cout, k, s, p, tr = geom
    x = _rand((B, Cin, H, W), 1).to(dtype)
    wshape = (Cin, Cout, k, k) if tr else (Cout, Cin, k, k)
    w = _rand(wshape, 2, 0.3).to(dtype)
    bias = _rand((Cout,), 3)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    fn = F.conv_transpose2d if tr else F.conv2d
    y64 = fn(x64, w64, bias.double(), stride=s, padding=p)
    dy = _rand(tuple(y64.shape), 4).to(dtype)
    y64.backward(dy.double())

    def rel(a, b):
        return ((a.cpu().double() - b).norm() / (b.norm() + 1e-30)).item()
    y = ops.conv_fwd(x.cuda(), w.cuda(), bias.cuda(), s, p, tr, torch.float32)
    assert tuple(y.shape) == tuple(y64.shape)
    assert rel(y, y64.detach()) < 1e-5, f'fwd {geom} {dtype}'
    dx = ops.conv_dgrad(dy.cuda(), w.cuda(), x.shape, s, p, tr, torch.float32)
    assert rel(dx, x64.grad) < 1e-5, f'dgrad {geom} {dtype}'
    dw = ops.conv_wgrad(dy.cuda(), x.cuda(), wshape, s, p, tr)
    assert rel(dw, w64.grad) < 1e-5, f'wgrad {geom} {dtype}'
    if tr:
        # the order functional.ConvBlock.backward uses: weight gradient, then the input gradient reusing its column matrix
        dx2 = ops.conv_dgrad(dy.cuda(), w.cuda(), x.shape, s, p, tr, torch.float32, cols_from_wgrad=True)
        assert rel(dx2, x64.grad) < 1e-5, f'dgrad after wgrad {geom} {dtype}'
    # with and without the transient column matrix: same contraction, same operands -> same numbers up to summation order
    import os
    os.environ['VS_CONV_COLS'] = '0'
    try:
        y0 = ops.conv_fwd(x.cuda(), w.cuda(), bias.cuda(), s, p, tr, torch.float32)
    finally:
        del os.environ['VS_CONV_COLS']
    assert rel(y0, y64.detach()) < 1e-5


@pytest.mark.parametrize('act', ['leaky_relu', 'relu', 'none', 'sigmoid'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
def test_batchnorm_act_fwd_bwd(act, dtype):
    from spatiotemporal_variable_separation_amd import ops
    B, C, H, W = 5, 7, 12, 10
    x = (_rand((B, C, H, W), 11) * 2 + 0.3).to(dtype)
    gamma, beta = 1 + _rand((C,), 12, 0.3), _rand((C,), 13, 0.2)
    dy = _rand((B, C, H, W), 14)
    rm, rv = _rand((C,), 15, 0.1), 1 + _rand((C,), 16, 0.2)
    bn = torch.nn.BatchNorm2d(C).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    acts = {'leaky_relu': lambda t: F.leaky_relu(t, 0.2), 'relu': torch.relu, 'none': lambda t: t, 'sigmoid': torch.sigmoid}
    x64 = x.double().requires_grad_(True)
    y64 = acts[act](bn(x64))
    y64.backward(dy.double())
    rmc, rvc = rm.clone().cuda(), rv.clone().cuda()
    xc = x.cuda()
    mean, invstd = ops.bn_stats(xc, rmc, rvc, 0.1, 1e-5)
    y = ops.bn_act_fwd(xc, mean, invstd, gamma.cuda(), beta.cuda(), act, torch.float32)
    dx, dg, db = ops.bn_act_bwd(dy.cuda(), xc, mean, invstd, gamma.cuda(), beta.cuda(), act, True, torch.float32)

    def rel(a, b):
        return ((a.cpu().double() - b).norm() / (b.norm() + 1e-30)).item()
    assert rel(y, y64.detach()) < 2e-6
    assert rel(rmc, bn.running_mean) < 2e-6 and rel(rvc, bn.running_var) < 2e-6
    assert rel(dx, x64.grad) < 2e-5
    assert rel(dg, bn.weight.grad) < 2e-5 and rel(db, bn.bias.grad) < 2e-5
    # 16 sequential calls update the running statistics sequentially
    for _ in range(15):
        bn(x64.detach())
        ops.bn_stats(xc, rmc, rvc, 0.1, 1e-5)
    assert rel(rmc, bn.running_mean) < 1e-5 and rel(rvc, bn.running_var) < 1e-5


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
def test_pool_upsample(dtype):
    from spatiotemporal_variable_separation_amd import ops
    x = _rand((3, 5, 8, 12), 21).to(dtype)
    x64 = x.double().requires_grad_(True)
    y64 = F.max_pool2d(x64, 2, 2)
    dy = _rand(tuple(y64.shape), 22).to(dtype)
    y64.backward(dy.double())
    y = ops.maxpool2_fwd(x.cuda())
    assert torch.equal(y.cpu().double(), y64.detach())
    dx = ops.maxpool2_bwd(x.cuda(), dy.cuda())
    assert torch.equal(dx.cpu().double(), x64.grad)
    x64b = x.double().requires_grad_(True)
    u64 = F.interpolate(x64b, scale_factor=2, mode='nearest')
    du = _rand(tuple(u64.shape), 23)
    u64.backward(du.double())
    u = ops.upsample2_fwd(x.cuda())
    assert torch.equal(u.cpu().double(), u64.detach())
    dxu = ops.upsample2_bwd(du.cuda(), torch.float32)
    assert ((dxu.cpu().double() - x64b.grad).norm() / x64b.grad.norm()).item() < 1e-6


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('shape', [(3, 5, 16, 16), (2, 7, 32, 64), (5, 3, 4, 48), (1, 2, 64, 32)])
def test_pool_upsample_16_byte_forms(dtype, shape):
    """The 16-byte kernels vs_maxpool2_* / vs_upsample2_* take for 16-bit tensors whose small-map rows are whole 16-byte pieces (the VGG
    encoders / decoders, conv.py:127-171, 296-314): forward results equal torch's on the same values bit for bit, the pooling gradient too
    (ties included: the first maximum in scan order wins), the upsampling gradient is the fp32 sum of four rounded once."""
    from spatiotemporal_variable_separation_amd import ops
    B, C, H, W = shape
    x = _rand(shape, 41).to(dtype)
    x[0, 0, :2, :4] = 0.5                                        # a window of equal values: the gradient goes to its first pixel
    x64 = x.double().requires_grad_(True)
    y64 = F.max_pool2d(x64, 2, 2)
    dy = _rand(tuple(y64.shape), 42).to(dtype)
    y64.backward(dy.double())
    y = ops.maxpool2_fwd(x.cuda())
    assert y.dtype == dtype and torch.equal(y.cpu().double(), y64.detach())
    dx = ops.maxpool2_bwd(x.cuda(), dy.cuda())
    assert dx.dtype == dtype and torch.equal(dx.cpu().double(), x64.grad)
    xs = x[:, :, :H // 2, :W // 2].contiguous()                  # (small map with rows of W / 2 >= 8 pixels)
    u = ops.upsample2_fwd(xs.cuda())
    assert u.dtype == dtype and torch.equal(u.cpu(), F.interpolate(xs.float(), scale_factor=2, mode='nearest').to(dtype))
    du = _rand(tuple(u.shape), 43).to(dtype)
    dxu = ops.upsample2_bwd(du.cuda(), dtype)
    d = du.float()
    want = (((d[:, :, 0::2, 0::2] + d[:, :, 0::2, 1::2]) + d[:, :, 1::2, 0::2]) + d[:, :, 1::2, 1::2]).to(dtype)
    assert dxu.dtype == dtype and torch.equal(dxu.cpu(), want)


def test_grouped_batchnorm_equals_sequential_calls():
    """groups = G on a stacked batch == G separate BatchNorm calls (statistics, outputs, gradients, running stats)."""
    from spatiotemporal_variable_separation_amd import ops
    G, Bg, C, H, W = 3, 4, 6, 8, 8
    x = (_rand((G * Bg, C, H, W), 31) * 1.5 + 0.2)
    dy = _rand((G * Bg, C, H, W), 32)
    gamma, beta = 1 + _rand((C,), 33, 0.3), _rand((C,), 34, 0.2)
    rm0, rv0 = _rand((C,), 35, 0.1), 1 + _rand((C,), 36, 0.2)
    xc, dyc = x.cuda(), dy.cuda()
    rm_g, rv_g = rm0.clone().cuda(), rv0.clone().cuda()
    mean, invstd = ops.bn_stats(xc, rm_g, rv_g, 0.1, 1e-5, groups=G)
    y = ops.bn_act_fwd(xc, mean, invstd, gamma.cuda(), beta.cuda(), 'leaky_relu', torch.float32, groups=G)
    dx, dg, db = ops.bn_act_bwd(dyc, xc, mean, invstd, gamma.cuda(), beta.cuda(), 'leaky_relu', True, torch.float32, groups=G)
    rm_s, rv_s = rm0.clone().cuda(), rv0.clone().cuda()
    dg_s, db_s = torch.zeros(C, device='cuda'), torch.zeros(C, device='cuda')
    for g in range(G):
        sl = slice(g * Bg, (g + 1) * Bg)
        xs = xc[sl].contiguous()
        m1, i1 = ops.bn_stats(xs, rm_s, rv_s, 0.1, 1e-5)
        y1 = ops.bn_act_fwd(xs, m1, i1, gamma.cuda(), beta.cuda(), 'leaky_relu', torch.float32)
        dx1, dg1, db1 = ops.bn_act_bwd(dyc[sl].contiguous(), xs, m1, i1, gamma.cuda(), beta.cuda(), 'leaky_relu', True, torch.float32)
        assert torch.equal(y[sl], y1) and torch.equal(dx[sl], dx1)
        dg_s += dg1
        db_s += db1
    assert torch.equal(rm_g, rm_s) and torch.equal(rv_g, rv_s)
    assert torch.allclose(dg, dg_s, rtol=1e-6, atol=1e-6) and torch.allclose(db, db_s, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('shape', [(2, 5, 33, 33), (3, 4, 8, 8), (1, 3, 5, 7), (2, 2, 1, 1)])
def test_maxpool3s2_matches_torch(dtype, shape):
    """nn.MaxPool2d(3, 2, 1) (ResNet18 stem): overlapping windows, gradient routed to the first maximum; ties included."""
    from spatiotemporal_variable_separation_amd import functional as VF
    x = (_rand(shape, 21) * 4).round() / 4                      # quarter steps: plenty of exact ties inside the windows
    x = x.to(dtype)
    xr = x.double().requires_grad_(True)
    yr = F.max_pool2d(xr, 3, 2, 1)
    dy = _rand(tuple(yr.shape), 22).to(dtype)
    yr.backward(dy.double())
    xd = x.cuda().requires_grad_(True)
    y = VF.MaxPool3s2.apply(xd)
    assert tuple(y.shape) == tuple(yr.shape) and torch.equal(y.cpu().double(), yr.detach())
    y.backward(dy.cuda())
    torch.testing.assert_close(xd.grad.cpu().double(), xr.grad, rtol=1e-2 if dtype != torch.float32 else 1e-6, atol=1e-2 if dtype != torch.float32 else 1e-6)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('shape,groups', [((6, 16, 17, 17), 1), ((4, 8, 9, 9), 2), ((3, 5, 33, 33), 1), ((8, 4, 3, 3), 2), ((2, 3, 5, 5), 1)])
def test_batchnorm_planes_not_a_multiple_of_the_vector_width(dtype, shape, groups):
    """The 17x17 / 9x9 / 33x33 maps of the chairs ResNet18: all tensors in one dtype take the unit-per-plane vector path
    (unaligned 16-byte accesses + a scalar tail); results against per-group fp64 BatchNorm of the same (rounded) inputs."""
    from spatiotemporal_variable_separation_amd import ops
    B, C, H, W = shape
    x = (_rand(shape, 31) * 2 + 0.3).to(dtype)
    dy = _rand(shape, 32).to(dtype)
    gamma, beta = 1 + _rand((C,), 33, 0.3), _rand((C,), 34, 0.2)
    xc, dyc = x.cuda(), dy.cuda()
    mean, invstd = ops.bn_stats(xc, groups=groups)
    y = ops.bn_act_fwd(xc, mean, invstd, gamma.cuda(), beta.cuda(), 'leaky_relu', dtype, groups=groups)
    dx, dg, db = ops.bn_act_bwd(dyc, xc, mean, invstd, gamma.cuda(), beta.cuda(), 'leaky_relu', True, dtype, groups=groups)
    ys, dxs, dgs, dbs = [], [], 0, 0
    per = B // groups
    for g in range(groups):
        bn = torch.nn.BatchNorm2d(C).double()
        with torch.no_grad():
            bn.weight.copy_(gamma); bn.bias.copy_(beta)
        xg = x[g * per:(g + 1) * per].double().requires_grad_(True)
        yg = F.leaky_relu(bn(xg), 0.2)
        yg.backward(dy[g * per:(g + 1) * per].double())
        ys.append(yg.detach()); dxs.append(xg.grad)
        dgs, dbs = dgs + bn.weight.grad, dbs + bn.bias.grad
    tol = 1e-2 if dtype != torch.float32 else 2e-5          # bf16: the OUTPUTS are stored in bf16

    def rel(a, b):
        return ((a.cpu().double() - b).norm() / (b.norm() + 1e-30)).item()
    assert rel(y, torch.cat(ys)) < tol and rel(dx, torch.cat(dxs)) < tol
    assert rel(dg, dgs) < 2e-5 and rel(db, dbs) < 2e-5       # fp32 sums of fp64-accumulated reductions
    if dtype != torch.float32:
        # mixed dtypes (bf16 activations, fp32 gradient in / out): 4-element units
        y32 = ops.bn_act_fwd(xc, mean, invstd, gamma.cuda(), beta.cuda(), 'leaky_relu', torch.float32, groups=groups)
        dx32, dg32, db32 = ops.bn_act_bwd(dyc.float(), xc, mean, invstd, gamma.cuda(), beta.cuda(), 'leaky_relu', True, torch.float32, groups=groups)
        assert rel(y32, torch.cat(ys)) < 2e-5 and rel(dx32, torch.cat(dxs)) < 2e-5
        assert rel(dg32, dgs) < 2e-5 and rel(db32, dbs) < 2e-5


# ---- ConvTranspose2d k4 s2 p1 as tap GEMM + col2im epilogue (csrc/vs_conv_tap.hip) ------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('geom', [
    # (B, Cin, H, Cout, groups)
    (32, 64, 4, 32, 2),       # 4x4 maps: 16 samples per 256-pixel tile
    (16, 128, 8, 64, 4),      # 8x8 maps: 4 samples per tile
    (6, 96, 16, 40, 3),       # 16x16 maps: one sample per tile; Cout not a multiple of 16, K = 96 (three K tiles)
    (48, 32, 4, 8, 1),        # a single K tile, 8 output channels (half an m-block)
    (20, 200, 8, 24, 5),      # K tail (200 = 6 x 32 + 8), last pixel tile partly empty (20 x 64 = 1280 = 5 x 256)
    (128, 512, 4, 256, 1),    # DCGAN decoder layer 1 at full width
])
def test_convt_tap_kernel_matches_fp64_and_yields_batchnorm_sums(dtype, geom):
    """Output = fp64 transposed convolution of the same rounded operands, rounded once to the storage type; the epilogue's fp64
    sums are those of the stored values per (call group, channel), so vs_bn_stats_from_sums reproduces vs_bn_stats."""
    from spatiotemporal_variable_separation_amd import ops
    B, Cin, H, Cout, groups = geom
    x = _rand((B, Cin, H, H), 41).to(dtype)
    w32 = _rand((Cin, Cout, 4, 4), 42, 0.3)
    w = w32.to(dtype)
    bias = _rand((Cout,), 43)
    xc = x.cuda()
    assert ops.convt_tap_supported(xc, Cout, groups)
    wt = ops.convt_tap_pack_weight(w.float().cuda(), dtype)
    y, sums = ops.convt_tap_fwd(xc, wt, bias.cuda(), Cout, groups=groups)
    torch.cuda.synchronize()
    ref = F.conv_transpose2d(x.double(), w.double(), bias.double(), stride=2, padding=1)
    assert tuple(y.shape) == tuple(ref.shape) and y.dtype == dtype
    want = ref.to(dtype)                                        # one rounding of the exact sum
    diff = (y.cpu().double() - want.double()).abs()
    ulp = (2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10) * want.double().abs().clamp_min(1e-3)     # >= one unit in the last place
    slack = 2e-6 * want.double().abs().max()                     # fp32 accumulation noise on near-zero sums (K up to 2048 products)
    assert (diff <= 1.01 * ulp + slack).all(), f'{geom} {dtype}: max {diff.max().item():.3e}'     # fp32 accumulation order: at most one ulp
    assert (diff > 0).double().mean().item() < 0.02, 'more than 2 % of the elements differ by an ulp'
    # sums of the STORED values
    ys = y.cpu().double().view(groups, B // groups, Cout, -1)
    s1, s2 = ys.sum(dim=(1, 3)), (ys * ys).sum(dim=(1, 3))
    got = sums.cpu()
    assert torch.allclose(got[..., 0], s1, rtol=1e-6, atol=1e-6) and torch.allclose(got[..., 1], s2, rtol=1e-6, atol=1e-6)
    rm, rv = torch.zeros(Cout).cuda(), torch.ones(Cout).cuda()
    rm2, rv2 = rm.clone(), rv.clone()
    mean, invstd = ops.bn_stats_from_sums(sums, (B // groups) * 4 * H * H, rm, rv, 0.1, 1e-5)
    mean2, invstd2 = ops.bn_stats(y, rm2, rv2, 0.1, 1e-5, groups=groups)
    assert torch.allclose(mean, mean2, rtol=1e-6, atol=1e-7) and torch.allclose(invstd, invstd2, rtol=1e-5)
    assert torch.allclose(rm, rm2, rtol=1e-6, atol=1e-7) and torch.allclose(rv, rv2, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('geom', [
    # (B, Cin, H, Cout, groups)
    (32, 64, 4, 40, 2),       # 4x4 maps (VGG encoder tail): 4-pixel work items
    (16, 128, 8, 64, 4),      # 8x8
    (5, 96, 16, 30, 1),       # 16x16, Cout = one full block of 28 + 2
    (8, 64, 16, 512, 1),      # ConvResBlock of the SST integrator, first conv (64 -> 512 at 16x16)
    (3, 520, 16, 64, 3),      # K tail (520 = 16 x 32 + 8), three call groups
])
def test_conv_k3_tap_kernel_forward_and_input_gradient(dtype, geom):
    """Conv2d k3 s1 p1 through the tap kernel: output (one rounding of the exact sum), BatchNorm sums of the stored values, fp32
    output form, and the input gradient via the flipped / transposed pack."""
    from spatiotemporal_variable_separation_amd import ops
    B, Cin, H, Cout, groups = geom
    x = _rand((B, Cin, H, H), 51).to(dtype)
    w32 = _rand((Cout, Cin, 3, 3), 52, 0.3)
    w = w32.to(dtype)
    bias = _rand((Cout,), 53)
    xc = x.cuda()
    assert ops.conv_k3_tap_supported(xc, Cout, groups, force=True)
    wt = ops.conv_k3_tap_pack_weight(w.float().cuda(), dtype, False)
    y, sums = ops.conv_k3_tap_fwd(xc, wt, bias.cuda(), Cout, dtype, groups=groups, want_sums=True)
    y32, _ = ops.conv_k3_tap_fwd(xc, wt, bias.cuda(), Cout, torch.float32)
    torch.cuda.synchronize()
    x64 = x.double().requires_grad_(True)
    ref = F.conv2d(x64, w.double(), bias.double(), stride=1, padding=1)
    want = ref.detach().to(dtype)
    diff = (y.cpu().double() - want.double()).abs()
    ulp = (2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10) * want.double().abs().clamp_min(1e-3)
    slack = 2e-6 * want.double().abs().max()
    assert (diff <= 1.01 * ulp + slack).all(), f'{geom} {dtype}: max {diff.max().item():.3e}'
    assert (diff > 0).double().mean().item() < 0.02
    assert ((y32.cpu().double() - ref.detach()).norm() / ref.detach().norm()).item() < 1e-5
    ys = y.cpu().double().view(groups, B // groups, Cout, -1)
    got = sums.cpu()
    assert torch.allclose(got[..., 0], ys.sum(dim=(1, 3)), rtol=1e-6, atol=1e-6) and torch.allclose(got[..., 1], (ys * ys).sum(dim=(1, 3)), rtol=1e-6, atol=1e-6)
    # input gradient: dz (16-bit) -> dx, fp32 and 16-bit outputs
    dz = _rand(tuple(ref.shape), 54).to(dtype)
    ref.backward(dz.double())
    if ops.conv_k3_tap_supported(dz.cuda(), Cin, 1, force=True):
        wtf = ops.conv_k3_tap_pack_weight(w.float().cuda(), dtype, True)
        dx, _ = ops.conv_k3_tap_fwd(dz.cuda(), wtf, None, Cin, torch.float32)
        assert ((dx.cpu().double() - x64.grad).norm() / x64.grad.norm()).item() < 1e-5, f'dgrad {geom} {dtype}'


@pytest.mark.parametrize('act', ['leaky_relu', 'relu'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('shape', [(8, 64, 16, 16), (3, 40, 8, 8), (8, 32, 32, 32), (2, 512, 4, 4), (5, 33, 8, 24)])
def test_batchnorm_small_slab_one_launch_paths(act, dtype, shape):
    """vs_bn_train_fwd_small (statistics + running update + affine + activation in ONE launch) and the one-launch backward that
    vs_bn_act_bwd takes for slabs of <= 8192 elements per channel (the SST integrator's maps), against torch's BatchNorm2d in
    fp64 on the same (rounded) inputs: outputs, running statistics after 1 and 16 sequential calls, all three gradients; and
    against the two-/three-launch kernels they replace."""
    import os
    from spatiotemporal_variable_separation_amd import ops
    B, C, H, W = shape
    x = (_rand(shape, 21) * 2 + 0.3).to(dtype)
    gamma, beta = 1 + _rand((C,), 22, 0.3), _rand((C,), 23, 0.2)
    dy = _rand(shape, 24).to(dtype)
    rm, rv = _rand((C,), 25, 0.1), 1 + _rand((C,), 26, 0.2)
    bn = torch.nn.BatchNorm2d(C).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    acts = {'leaky_relu': lambda t: F.leaky_relu(t, 0.2), 'relu': torch.relu}
    x64 = x.double().requires_grad_(True)
    y64 = acts[act](bn(x64))
    y64.backward(dy.double())
    xc, dyc = x.cuda(), dy.cuda()
    assert ops.bn_small_supported(xc), shape
    rmc, rvc = rm.clone().cuda(), rv.clone().cuda()
    y, mean, invstd = ops.bn_train_fwd_small(xc, gamma.cuda(), beta.cuda(), act, torch.float32, rmc, rvc, 0.1, 1e-5)
    dx, dg, db = ops.bn_act_bwd(dyc, xc, mean, invstd, gamma.cuda(), beta.cuda(), act, True, torch.float32)

    def rel(a, b):
        return ((a.cpu().double() - b.cpu().double()).norm() / (b.cpu().double().norm() + 1e-30)).item()
    assert rel(y, y64.detach()) < 2e-6
    assert rel(rmc, bn.running_mean) < 2e-6 and rel(rvc, bn.running_var) < 2e-6
    assert rel(dx, x64.grad) < 2e-5
    assert rel(dg, bn.weight.grad) < 2e-5 and rel(db, bn.bias.grad) < 2e-5
    # the kernels they replace (same results up to summation order); 16-bit outputs too
    rm2, rv2 = rm.clone().cuda(), rv.clone().cuda()
    m2, i2 = ops.bn_stats(xc, rm2, rv2, 0.1, 1e-5)
    assert rel(mean, m2) < 1e-6 and rel(invstd, i2) < 1e-6 and rel(rmc, rm2) < 1e-6 and rel(rvc, rv2) < 1e-6
    if dtype != torch.float32:
        y16 = ops.bn_train_fwd_small(xc, gamma.cuda(), beta.cuda(), act, dtype, None, None, 0.1, 1e-5)[0]
        assert rel(y16, y64.detach()) < (6e-3 if dtype == torch.bfloat16 else 8e-4)
        dx16 = ops.bn_act_bwd(dyc, xc, mean, invstd, gamma.cuda(), beta.cuda(), act, True, dtype)[0]
        assert rel(dx16, x64.grad) < (6e-3 if dtype == torch.bfloat16 else 8e-4)
    for _ in range(15):
        bn(x64.detach())
        ops.bn_train_fwd_small(xc, gamma.cuda(), beta.cuda(), act, torch.float32, rmc, rvc, 0.1, 1e-5)
    assert rel(rmc, bn.running_mean) < 1e-5 and rel(rvc, bn.running_var) < 1e-5


@pytest.mark.parametrize('act', ['leaky_relu', 'none', 'relu'])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('shape,groups', [((16, 24, 32, 32), 1), ((128, 8, 32, 32), 1), ((96, 6, 16, 16), 2), ((33, 5, 32, 32), 3), ((8, 9, 64, 64), 2),
                                          ((40, 3, 16, 64), 1), ((63, 4, 32, 32), 1), ((200, 3, 32, 32), 2), ((88, 3, 32, 32), 1), ((30, 2, 64, 64), 1)])
def test_batchnorm_register_resident_slabs(act, dtype, shape, groups):
    """vs_bn_train_fwd_slab (a call's channel slab of 8 193 .. 131 072 16-bit elements read ONCE and held in registers: statistics, running
    update, affine + activation) and the resident backward vs_bn_act_bwd takes for slabs up to 65 536 elements, per call group against torch's
    BatchNorm2d in fp64 on the same (rounded) inputs; forward also against vs_bn_stats + vs_bn_act_fwd, the launches it replaces."""
    from spatiotemporal_variable_separation_amd import ops
    B, C, H, W = shape
    Bg = B // groups
    x = (_rand(shape, 31) * 2 + 0.3).to(dtype)
    gamma, beta = 1 + _rand((C,), 32, 0.3), _rand((C,), 33, 0.2)
    dy = _rand(shape, 34).to(dtype)
    rm, rv = _rand((C,), 35, 0.1), 1 + _rand((C,), 36, 0.2)
    bn = torch.nn.BatchNorm2d(C).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    acts = {'leaky_relu': lambda t: F.leaky_relu(t, 0.2), 'relu': torch.relu, 'none': lambda t: t}
    x64 = x.double().requires_grad_(True)
    y64 = torch.cat([acts[act](bn(x64[g * Bg:(g + 1) * Bg])) for g in range(groups)])          # (one reference call per group, in order)
    y64.backward(dy.double())
    xc, dyc = x.cuda(), dy.cuda()
    assert ops.bn_slab_supported(xc, groups), shape
    rmc, rvc = rm.clone().cuda(), rv.clone().cuda()
    y, mean, invstd = ops.bn_train_fwd_slab(xc, gamma.cuda(), beta.cuda(), act, torch.float32, rmc, rvc, 0.1, 1e-5, groups=groups)
    assert mean.shape == (groups, C) and invstd.shape == (groups, C)

    def rel(a, b):
        return ((a.cpu().double() - b.cpu().double()).norm() / (b.cpu().double().norm() + 1e-30)).item()
    assert rel(y, y64.detach()) < 2e-6
    assert rel(rmc, bn.running_mean) < 2e-6 and rel(rvc, bn.running_var) < 2e-6
    rm2, rv2 = rm.clone().cuda(), rv.clone().cuda()
    m2, i2 = ops.bn_stats(xc, rm2, rv2, 0.1, 1e-5, groups=groups)
    assert rel(mean, m2) < 1e-6 and rel(invstd, i2) < 1e-6 and rel(rmc, rm2) < 1e-6 and rel(rvc, rv2) < 1e-6
    y16 = ops.bn_train_fwd_slab(xc, gamma.cuda(), beta.cuda(), act, dtype, None, None, 0.1, 1e-5, groups=groups)[0]
    y16_2 = ops.bn_act_fwd(xc, m2, i2, gamma.cuda(), beta.cuda(), act, dtype, groups=groups)
    assert rel(y16, y64.detach()) < (6e-3 if dtype == torch.bfloat16 else 8e-4)
    assert (y16.float() - y16_2.float()).abs().max().item() <= 2e-2 * y16_2.float().abs().max().item()      # (an ulp where the statistics differ in their last bit)
    # backward (slabs <= 65 536 elements: x and dy in registers; up to 131 072: x in registers, dy in LDS + a tail read twice)
    dx, dg, db = ops.bn_act_bwd(dyc, xc, mean, invstd, gamma.cuda(), beta.cuda(), act, True, torch.float32, groups=groups)
    assert rel(dx, x64.grad) < 2e-5
    assert rel(dg, bn.weight.grad) < 2e-5 and rel(db, bn.bias.grad) < 2e-5
    dx16 = ops.bn_act_bwd(dyc, xc, mean, invstd, gamma.cuda(), beta.cuda(), act, True, dtype, groups=groups)[0]
    assert rel(dx16, x64.grad) < (6e-3 if dtype == torch.bfloat16 else 8e-4)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('transposed,geom', [(False, (8, 64, 16, 512, 3, 1, 1)), (False, (4, 24, 16, 40, 4, 2, 1)), (True, (6, 32, 8, 16, 4, 2, 1))])
def test_conv_wgrad_accumulates_into_an_existing_gradient(dtype, transposed, geom):
    """ops.conv_wgrad(..., into=g): g += dW in the GEMM / split-K epilogue == g + conv_wgrad(...) (the integrator's blocks add one
    contribution per predicted frame)."""
    from spatiotemporal_variable_separation_amd import ops
    B, Cin, H, Cout, k, stride, pad = geom
    x = _rand((B, Cin, H, H), 31).to(dtype).cuda()
    OH = (H - 1) * stride - 2 * pad + k if transposed else (H + 2 * pad - k) // stride + 1
    dy = _rand((B, Cout, OH, OH), 32).to(dtype).cuda()
    w_shape = (Cin, Cout, k, k) if transposed else (Cout, Cin, k, k)
    base = _rand(w_shape, 33).cuda()
    fresh = ops.conv_wgrad(dy, x, w_shape, stride, pad, transposed)
    acc = base.clone()
    ops.conv_wgrad(dy, x, w_shape, stride, pad, transposed, into=acc)
    ops.conv_wgrad(dy, x, w_shape, stride, pad, transposed, into=acc)
    torch.cuda.synchronize()
    ref = base.double() + 2 * fresh.double()
    assert ((acc.double() - ref).norm() / ref.norm()).item() < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('geom', [
    (8, 512, 512),            # ConvResBlock of the SST integrator (resnet.py:53-70), middle conv: 2 splits of 256 channels
    (8, 64, 512),             # first conv: one split, one pass of 12 fragment groups
    (8, 512, 64),             # last conv: 8 splits of 64 channels
    (3, 128, 40),             # ragged output-channel tile (40 = 32 + 8), 2 splits
    (1, 192, 96),             # 192 channels in one split (three passes), a single map
    (32, 64, 33),             # the largest batch the few-maps path takes
])
def test_conv3_img16_forward_and_input_gradient(dtype, geom):
    """Conv2d k3 s1 p1 on a few 16x16 maps through vs_conv3_img16 (split slabs) + vs_slab_sum: against fp64 conv2d on the same 16-bit
    operands, the sum of the slabs without bias, the 16-bit output rounding, and the input gradient via the flipped / transposed pack."""
    from spatiotemporal_variable_separation_amd import ops, _lib
    B, Cin, Cout = geom
    x = _rand((B, Cin, 16, 16), 61).to(dtype)
    w = _rand((Cout, Cin, 3, 3), 62, 0.3).to(dtype)
    bias = _rand((Cout,), 63)
    xc = x.cuda()
    assert ops.conv3_img16_supported(xc, Cout)
    wp = ops.conv3_img16_pack_weight(w.float().cuda(), dtype, False)
    slabs = ops.conv3_img16(xc, wp, Cout)
    assert slabs.shape == (_lib.load_library().vs_conv3_img16_splits(B, Cin, Cout), B, Cout, 16, 16)
    y32 = ops.slab_sum(slabs, bias.cuda(), torch.float32)
    y16 = ops.slab_sum(slabs, bias.cuda(), dtype)
    torch.cuda.synchronize()
    x64 = x.double().requires_grad_(True)
    ref = F.conv2d(x64, w.double(), bias.double(), stride=1, padding=1)
    assert ((y32.cpu().double() - ref.detach()).norm() / ref.detach().norm()).item() < 1e-5
    assert ((slabs.sum(0).cpu().double() + bias.double().view(1, -1, 1, 1) - ref.detach()).norm() / ref.detach().norm()).item() < 1e-5
    assert torch.equal(y16.cpu(), y32.cpu().to(dtype))
    dz = _rand(tuple(ref.shape), 64).to(dtype)
    ref.backward(dz.double())
    if ops.conv3_img16_supported(dz.cuda(), Cin):
        wf = ops.conv3_img16_pack_weight(w.float().cuda(), dtype, True)
        dx = ops.slab_sum(ops.conv3_img16(dz.cuda(), wf, Cin), None, torch.float32)
        assert ((dx.cpu().double() - x64.grad).norm() / x64.grad.norm()).item() < 1e-5, f'dgrad {geom} {dtype}'


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('shape', [(3, 8, 64), (2, 8, 512), (8, 2, 40)])
def test_batchnorm_small_from_split_slabs_equals_sum_then_batchnorm(dtype, shape):
    """vs_bn_train_fwd_small_slabs == vs_slab_sum (bias, 16-bit rounding) followed by vs_bn_train_fwd_small, bit for bit: z, y, batch
    statistics and running statistics."""
    from spatiotemporal_variable_separation_amd import ops
    S, B, C = shape
    slabs = _rand((S, B, C, 16, 16), 71).cuda()
    bias = _rand((C,), 72).cuda()
    gamma, beta = (1 + _rand((C,), 73, 0.3)).cuda(), _rand((C,), 74, 0.2).cuda()
    rm1, rv1 = _rand((C,), 75, 0.1).cuda(), (1 + _rand((C,), 76, 0.2)).cuda()
    rm2, rv2 = rm1.clone(), rv1.clone()
    y1, z1, m1, i1 = ops.bn_train_fwd_small_slabs(slabs, bias, dtype, gamma, beta, 'leaky_relu', dtype, rm1, rv1, 0.1, 1e-5)
    z2 = ops.slab_sum(slabs, bias, dtype)
    y2, m2, i2 = ops.bn_train_fwd_small(z2, gamma, beta, 'leaky_relu', dtype, rm2, rv2, 0.1, 1e-5)
    torch.cuda.synchronize()
    assert torch.equal(z1, z2) and torch.equal(y1, y2)
    assert torch.equal(m1, m2) and torch.equal(i1, i2) and torch.equal(rm1, rm2) and torch.equal(rv1, rv2)
    y3 = ops.bn_train_fwd_small_slabs(slabs, None, dtype, gamma, beta, 'none', torch.float32, None, None, 0.1, 1e-5)[0]
    assert y3.dtype == torch.float32 and torch.isfinite(y3).all()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('geom', [(8, 64, 512), (8, 512, 512), (8, 512, 64), (3, 128, 96), (5, 256, 40)])
def test_conv3_img16_bn_one_launch_layer_matches_two_launches(dtype, geom, monkeypatch):
    """vs_conv3_img16_bn_fwd / _bwd (convolution + BatchNorm of a ConvResBlock layer in ONE launch; partial sums of the input-channel splits and
    the per-map statistics exchanged inside the launch) against vs_conv3_img16 + vs_bn_train_fwd_small_slabs / vs_bn_act_bwd_small_ex: z bit for
    bit (same sums in the same order), statistics to 2e-6, y / dz equal except isolated values on a rounding boundary, running estimates and
    parameter gradients to 1e-5; the 64 -> 512, 512 -> 512 (two splits) and 512 -> 64 (eight splits) geometries of the SST integrator, ragged
    channel tiles, a repeated launch (new epoch) bit-identical, no exchange time-out."""
    from spatiotemporal_variable_separation_amd import ops
    monkeypatch.setenv('VS_IMG_BN_SPLITS', '1,2,8')           # (the default serves unsplit layers only: see ops.conv3_img16_bn_supported)
    B, Cin, Cout = geom
    if not ops.conv3_img16_bn_supported(B, Cin, Cout, dtype):
        pytest.skip('geometry not served by the one-launch layer')
    x = _rand((B, Cin, 16, 16), 601).to(dtype).cuda()
    w = _rand((Cout, Cin, 3, 3), 602, 0.2).cuda()
    bias = _rand((Cout,), 603).cuda()
    gamma, beta = (1 + _rand((Cout,), 604, 0.3)).cuda(), _rand((Cout,), 605, 0.2).cuda()
    skip = _rand((B, Cout, 16, 16), 606).cuda()
    wp = ops.conv3_img16_pack_weight(w, dtype, False)
    rm1, rv1 = _rand((Cout,), 607, 0.1).cuda(), (1 + _rand((Cout,), 608, 0.2)).cuda()
    rm2, rv2 = rm1.clone(), rv1.clone()
    slabs = ops.conv3_img16(x, wp, Cout)
    # the block's last layer: no activation, fp32 output, skip added
    y0, z0, m0, i0, xn0, xn16_0 = ops.bn_train_fwd_small_slabs(slabs, bias, dtype, gamma, beta, 'none', torch.float32, rm1, rv1, 0.1, 1e-5, skip=skip, want16=True)
    y1, z1, m1, i1, xn1, xn16_1 = ops.conv3_img16_bn_fwd(x, wp, bias, gamma, beta, 'none', torch.float32, Cout, rm2, rv2, 0.1, 1e-5, skip=skip, want16=True)
    rm3, rv3 = rm2.clone(), rv2.clone()
    again = ops.conv3_img16_bn_fwd(x, wp, bias, gamma, beta, 'none', torch.float32, Cout, rm3, rv3, 0.1, 1e-5, skip=skip, want16=True)
    torch.cuda.synchronize()
    assert ops.rollout_exchange_error(x.device) == 0
    assert torch.equal(z1, z0)
    assert torch.allclose(m1, m0, rtol=2e-6, atol=2e-7) and torch.allclose(i1, i0, rtol=2e-6, atol=0)
    assert torch.allclose(y1, y0, rtol=1e-5, atol=1e-5) and torch.allclose(xn1, xn0, rtol=1e-5, atol=1e-5)
    assert (xn16_1 != xn16_0).float().mean().item() < 1e-3
    assert torch.allclose(rm2, rm1, rtol=1e-6, atol=1e-7) and torch.allclose(rv2, rv1, rtol=1e-5, atol=1e-7)
    assert torch.equal(again[0], y1) and torch.equal(again[1], z1) and torch.equal(again[2], m1)          # reproducible, epochs move on
    # 16-bit output of an inner layer
    y16_0 = ops.bn_train_fwd_small_slabs(slabs, bias, dtype, gamma, beta, 'leaky_relu', dtype, None, None, 0.1, 1e-5)[0]
    y16_1 = ops.conv3_img16_bn_fwd(x, wp, bias, gamma, beta, 'leaky_relu', dtype, Cout)[0]
    assert (y16_1 != y16_0).float().mean().item() < 1e-3
    # backward layer: dz_next has Cnext channels, the layer above maps Cout -> Cnext
    Cnext = Cin                                               # (any supported pair: reuse the geometry mirrored)
    if not ops.conv3_img16_bn_supported(B, Cnext, Cout, dtype):
        return
    w_up = _rand((Cnext, Cout, 3, 3), 609, 0.2).cuda()
    wf = ops.conv3_img16_pack_weight(w_up, dtype, True)
    dz_next = _rand((B, Cnext, 16, 16), 610).to(dtype).cuda()
    sl = ops.conv3_img16(dz_next, wf, Cout, role='dgrad')
    d0, dg0, db0 = ops.bn_act_bwd_small_ex(z0, m0, i0, gamma, beta, 'leaky_relu', dtype, slabs=sl)
    d1, dg1, db1 = ops.conv3_img16_bn_bwd(dz_next, wf, Cout, z0, m0, i0, gamma, beta, 'leaky_relu')
    pend_g, pend_b = _rand((Cout,), 611).cuda(), _rand((Cout,), 612).cuda()
    acc_g, acc_b = pend_g.clone(), pend_b.clone()
    d2, _, _ = ops.conv3_img16_bn_bwd(dz_next, wf, Cout, z0, m0, i0, gamma, beta, 'leaky_relu', acc=(acc_g, acc_b))
    torch.cuda.synchronize()
    assert ops.rollout_exchange_error(x.device) == 0
    scale = d0.float().abs().max().item()
    assert ((d1.float() - d0.float()).abs() > 1e-5 * scale).float().mean().item() < 2e-3
    assert ((d1.float() - d0.float()).norm() / d0.float().norm()).item() < 1e-3
    assert torch.allclose(dg1, dg0, rtol=1e-5, atol=1e-5 * dg0.abs().max().item()) and torch.allclose(db1, db0, rtol=1e-5, atol=1e-5 * db0.abs().max().item())
    assert torch.equal(d2, d1) and torch.allclose(acc_g, pend_g + dg1, rtol=1e-6, atol=1e-6) and torch.allclose(acc_b, pend_b + db1, rtol=1e-6, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['1', '2'])
@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_fused_conv_res_block_equals_layer_by_layer(precision, mode, monkeypatch):
    """ConvResBlock (resnet.py:53-70) through functional.ConvResBlockFn against the same block run layer by layer.  mode 1 (round 3: 6 launches
    forward, 7 backward, the same kernels as the layered path): forward outputs and running statistics bit for bit, gradients to the tolerance
    of the one difference -- the fused backward hands the inner BatchNorms the fp32 input gradient, the layered one a 16-bit rounding of it.
    mode 2 (round 4: ONE launch per layer, the statistics combined from per-map sums by the parallel-variance formula instead of one two-pass
    reduction): the stored pre-BatchNorm values are the same bits, mean / invstd agree to ~1e-7, so outputs agree except where that moves a
    value across a 16-bit rounding boundary (bounded below).  A second chained block re-uses the 16-bit copy of the first one's output."""
    import copy
    from spatiotemporal_variable_separation_amd import functional as VF
    from spatiotemporal_variable_separation_amd.networks.conv import ConvResnet
    with VF.precision(precision):
        torch.manual_seed(5)
        net = ConvResnet(64, n_blocks=2, nf=128).cuda().train()
        ref = copy.deepcopy(net)
        x0 = _rand((4, 64, 16, 16), 81).cuda()
        ga, gb = _rand((4, 64, 16, 16), 82).cuda(), _rand((4, 64, 16, 16), 83).cuda()
        outs = []
        monkeypatch.setenv('VS_IMG_BN_SPLITS', '1,2,8')
        for fused, m in ((mode, net), ('0', ref)):
            monkeypatch.setenv('VARSEP_FUSED_RESBLOCK', fused)
            x = x0.clone().requires_grad_(True)
            y, residuals = m(x)
            assert hasattr(y, '_vs16') == (fused != '0')          # the fused path leaves the 16-bit copy of its output
            (y * ga).sum().add((residuals[0] * gb).sum()).add((residuals[1] * ga).sum()).backward()
            torch.cuda.synchronize()
            outs.append((y.detach(), [r.detach() for r in residuals], x.grad))
        (y1, r1, g1), (y2, r2, g2) = outs
        from spatiotemporal_variable_separation_amd import ops
        assert ops.rollout_exchange_error(torch.device('cuda', torch.cuda.current_device())) == 0
        if mode == '1':
            assert torch.equal(y1, y2) and torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
            for (n1, b1), (_, b2) in zip(net.named_buffers(), ref.named_buffers()):
                assert torch.equal(b1, b2), n1
        else:
            ulp = 2.0 ** -8 if precision == 'bf16' else 2.0 ** -11
            for a, bb in ((y1, y2), (r1[0], r2[0]), (r1[1], r2[1])):
                d = (a - bb).abs()
                print(precision, 'one launch per layer vs layered: relative L2 %.2e, share of elements that moved %.2e' % (
                    (d.norm() / bb.norm()).item(), (d > 1e-5 * bb.abs().max()).float().mean().item()))
                # (a value that flips by one ulp in an inner layer flips roundings downstream: fp16, whose ulp is 8 x finer, sees ~1e-4 here)
                assert (d.norm() / bb.norm()).item() < 16 * ulp
            for (n1, b1), (_, b2) in zip(net.named_buffers(), ref.named_buffers()):
                assert torch.allclose(b1.float(), b2.float(), rtol=2e-3, atol=1e-4), n1
        tol = 3e-2 if mode == '2' else (2e-2 if precision == 'bf16' else 3e-3)

        def rel(a, b):
            return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()
        assert rel(g1, g2) < tol
        for (n1, p1), (_, p2) in zip(net.named_parameters(), ref.named_parameters()):
            if p2.grad.abs().max().item() == 0:
                assert p1.grad.abs().max().item() == 0, n1          # conv biases in front of BatchNorm
            else:
                assert rel(p1.grad, p2.grad) < tol, (n1, rel(p1.grad, p2.grad))


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_conv_res_block_output_kept_and_passed_on_joins_its_gradients_in_the_block(precision):
    """A rollout keeps every code AND feeds it to the next block-step (model.py:76-86).  The fused ConvResBlock hands its output out twice
    (`return_alias=True`): with the kept copy taken from the alias, the two gradients reach the block separately and join inside its backward launches
    (second upstream operand of the BatchNorm backward, second addend of the skip gradient); with the same tensor used twice autograd adds them
    first.  Same forward bits; gradients equal up to the order of two fp32 additions."""
    from spatiotemporal_variable_separation_amd import functional as VF
    from spatiotemporal_variable_separation_amd.networks.conv import ConvResnet
    with VF.precision(precision):
        torch.manual_seed(6)
        net = ConvResnet(64, n_blocks=1, nf=64).cuda().train()
        x0 = _rand((8, 64, 16, 16), 91).cuda()
        gs = [_rand((8, 64, 16, 16), 92 + i).cuda() for i in range(3)]
        res = []
        for use_alias in (True, False):
            net.zero_grad()
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.reset_running_stats()
            x = x0.clone().requires_grad_(True)
            kept, cur = [], x
            for _ in range(3):
                cur, _, alias = net(cur, return_alias=True)
                assert alias is not None and not hasattr(cur, '_vs_alias')
                kept.append(alias if use_alias else cur)
            sum((k * g).sum() for k, g in zip(kept, gs)).backward()
            torch.cuda.synchronize()
            res.append(([k.detach().clone() for k in kept], x.grad.clone(), [p.grad.clone() for p in net.parameters()]))
        (k1, dx1, p1), (k2, dx2, p2) = res
        for a, b in zip(k1, k2):
            assert torch.equal(a, b)

        def rel(a, b):
            return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()
        tol = 2e-2 if precision == 'bf16' else 3e-3                  # (an fp32 sum in another order re-rounds 16-bit dz values downstream)
        assert rel(dx1, dx2) < tol
        for a, b in zip(p1, p2):
            if b.abs().max().item() == 0:
                assert a.abs().max().item() == 0
            else:
                assert rel(a, b) < tol


@pytest.mark.gpu
def test_fused_conv_res_block_calls_do_not_leak():
    """Advisor finding (round 4): the block's second output used to hang on the tensor it is a view of (`xnew._vs_alias = alias`): a reference
    cycle through the C++ base pointer that `gc` cannot collect -- one fp32 [B, C, 16, 16] map (and its backward node) leaked per block call
    under grad.  The alias now travels through the return value; eager rollouts must leave `memory_allocated()` flat."""
    import gc
    from spatiotemporal_variable_separation_amd import functional as VF
    from spatiotemporal_variable_separation_amd.networks.conv import ConvResnet
    with VF.precision('bf16'):
        torch.manual_seed(7)
        net = ConvResnet(64, n_blocks=2, nf=64).cuda().train()
        x0 = _rand((8, 64, 16, 16), 17).cuda()

        def rollout():
            x = x0.clone().requires_grad_(True)
            kept, cur = [], x
            for _ in range(6):
                cur, _, alias = net(cur, return_alias=True)
                kept.append(alias)
            sum(k.sum() for k in kept).backward()
            net.zero_grad(set_to_none=True)

        for _ in range(3):
            rollout()
        gc.collect()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        for _ in range(10):
            rollout()
        gc.collect()
        torch.cuda.synchronize()
        grown = torch.cuda.memory_allocated() - base
        assert grown < 8 * 64 * 256 * 4, 'eager fused ConvResBlock calls leak %d bytes over 10 rollouts' % grown


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('geom', [
    (2, 64, 64, 64, 64),      # one phase, W = 64 (the two column tiles of a wave are the halves of one row)
    (3, 128, 32, 32, 40),     # two phases, W = 32, ragged output-channel tile
    (5, 192, 16, 16, 96),     # three phases, W = 16 (a column tile = two rows)
    (2, 64, 8, 64, 33),       # H != W: two bands of four rows
    (70, 256, 16, 16, 64),    # more workgroups than CUs: fragment loads still in flight when a workgroup ends
    (9, 128, 64, 64, 32),
    (10, 128, 8, 8, 72),      # 8 x 8 maps, four per workgroup: 10 = 2 full groups + 2 maps
    (3, 256, 8, 8, 256),
    (37, 128, 4, 4, 72),      # 4 x 4 maps, sixteen per workgroup: 37 = 2 full groups + 5 maps; ragged output-channel tile
    (16, 64, 4, 4, 64),       # one phase, one buffer
    (200, 512, 4, 4, 512),    # the VGG encoder's 512-channel layers at TaxiBJ size (conv.py:147-160)
    (6, 260, 16, 16, 256),    # channels not a multiple of 64 (SST decoder first layer, 256 + 4: conv.py:404): the last phase stages zeros
    (5, 24, 32, 32, 64),      # fewer than 64 input channels: one partial phase
    (3, 16, 64, 64, 48),      # (below 16 channels on either side the thin-channel kernels keep the layer: ops.conv3_band_supported)
    (9, 100, 8, 8, 40),       # 8 x 8 maps, ragged channels both ways
    (37, 40, 4, 4, 24),       # 4 x 4 maps, one partial phase
    (20, 96, 4, 4, 32),       # 4 x 4 maps, two phases (the second half empty)
    (7, 32, 8, 8, 16),
    (4, 16, 16, 16, 16),
])
def test_conv3_band_forward_and_input_gradient(dtype, geom):
    """Conv2d k3 s1 p1 on many maps through vs_conv3_band (row bands in LDS, no column matrix) against fp64 conv2d on the same 16-bit
    operands: fp32 output, the 16-bit output rounding, launch-to-launch reproducibility, and the input gradient (flipped pack)."""
    from spatiotemporal_variable_separation_amd import ops
    B, Cin, H, W, Cout = geom
    x = _rand((B, Cin, H, W), 91).to(dtype)
    w = _rand((Cout, Cin, 3, 3), 92, 0.3).to(dtype)
    bias = _rand((Cout,), 93)
    xc = x.cuda()
    assert ops.conv3_band_supported(xc, Cout)
    wp = ops.conv3_img16_pack_weight(w.float().cuda(), dtype, False)
    y32 = ops.conv3_band(xc, wp, bias.cuda(), Cout, torch.float32)
    y16 = ops.conv3_band(xc, wp, bias.cuda(), Cout, dtype)
    again = ops.conv3_band(xc, wp, bias.cuda(), Cout, torch.float32)
    torch.cuda.synchronize()
    x64 = x.double().requires_grad_(True)
    ref = F.conv2d(x64, w.double(), bias.double(), stride=1, padding=1)
    assert ((y32.cpu().double() - ref.detach()).norm() / ref.detach().norm()).item() < 1e-5
    assert ((y32.cpu().double() - ref.detach()).abs().max() / ref.detach().abs().max()).item() < 1e-5
    assert torch.equal(y16.cpu(), y32.cpu().to(dtype)) and torch.equal(again, y32)
    dz = _rand(tuple(ref.shape), 94).to(dtype)
    ref.backward(dz.double())
    if ops.conv3_band_supported(dz.cuda(), Cin):
        wf = ops.conv3_img16_pack_weight(w.float().cuda(), dtype, True)
        dx = ops.conv3_band(dz.cuda(), wf, None, Cin, torch.float32)
        assert ((dx.cpu().double() - x64.grad).abs().max() / x64.grad.abs().max()).item() < 1e-5, f'dgrad {geom} {dtype}'


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('geom', [
    (2, 64, 64, 64, 64),      # W = 64: four-row bands
    (3, 128, 32, 32, 40),     # ragged output-channel tile
    (5, 96, 16, 16, 72),      # W = 16, 3 x 3 tiles of 32 channels
    (2, 40, 8, 64, 33),       # ragged both ways, H != W
    (40, 64, 32, 32, 64),     # several bands per workgroup share
    (312, 64, 16, 16, 512),   # the SST integrator's batched call (39 x 8 maps)
    (10, 128, 8, 8, 72),      # 8 x 8 maps, four per item: two full items + two maps
    (9, 40, 8, 8, 256),
    (200, 512, 4, 4, 512),    # 4 x 4 maps, sixteen per item (the VGG encoders' 512-channel layers on the two stacked calls): 12 items + 8 maps
    (37, 40, 4, 4, 72),       # 4 x 4 maps, ragged channels both ways, a partial last item
    (5, 64, 4, 4, 24),        # fewer maps than one item
])
def test_conv3_wgrad_band_matches_fp64(dtype, geom, monkeypatch):
    """Weight gradient of Conv2d k3 s1 p1 through vs_conv3_wgrad_band + vs_slab_sum (ops.conv_wgrad picks it) against fp64 autograd on the
    same 16-bit operands, fresh and accumulated into a pending gradient; equal to the column-matrix path up to summation order."""
    from spatiotemporal_variable_separation_amd import ops
    monkeypatch.setenv('VS_CONV_WGRAD_BAND', '1')
    B, Cin, H, W, Cout = geom
    x = _rand((B, Cin, H, W), 101).to(dtype)
    dz = _rand((B, Cout, H, W), 102).to(dtype)
    assert ops.conv3_wgrad_band_supported(x.cuda(), Cout)
    w64 = torch.zeros((Cout, Cin, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w64, None, stride=1, padding=1).backward(dz.double())
    dw = ops.conv_wgrad(dz.cuda(), x.cuda(), (Cout, Cin, 3, 3), 1, 1, False)
    again = ops.conv_wgrad(dz.cuda(), x.cuda(), (Cout, Cin, 3, 3), 1, 1, False)
    pend = _rand((Cout, Cin, 3, 3), 103).cuda()
    acc = ops.conv_wgrad(dz.cuda(), x.cuda(), (Cout, Cin, 3, 3), 1, 1, False, into=pend.clone())
    torch.cuda.synchronize()
    scale = w64.grad.abs().max()
    assert ((dw.cpu().double() - w64.grad).abs().max() / scale).item() < 2e-6, geom
    assert torch.equal(dw, again)
    assert ((acc.cpu().double() - (w64.grad + pend.cpu().double())).abs().max() / scale).item() < 2e-6


@pytest.mark.gpu
def test_conv3_wgrad_band_over_separate_pieces_equals_the_concatenated_batch():
    """vs_conv3_wgrad_band_pieces (the remembered (dz, x) pairs of a repeatedly applied convolution, addressed where they lie) == the same
    kernel on the concatenation, bit for bit, fresh and accumulated."""
    from spatiotemporal_variable_separation_amd import ops
    dtype = torch.bfloat16
    pairs = [(_rand((8, 256, 16, 16), 200 + i).to(dtype).cuda(), _rand((8, 128, 16, 16), 300 + i).to(dtype).cuda()) for i in range(5)]
    shape = (256, 128, 3, 3)
    dz, x = torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])
    assert ops.conv3_wgrad_band_supported(x, 256)
    want = ops.conv_wgrad(dz, x, shape, 1, 1, False)
    got = ops.conv3_wgrad_band_pieces(pairs, shape)
    pend = _rand(shape, 77).cuda()
    acc_want = ops.conv_wgrad(dz, x, shape, 1, 1, False, into=pend.clone())
    acc_got = ops.conv3_wgrad_band_pieces(pairs, shape, into=pend.clone())
    torch.cuda.synchronize()
    assert got is not None and torch.equal(got, want) and torch.equal(acc_got, acc_want)
    assert ops.conv3_wgrad_band_pieces(pairs * 13, shape) is None            # more than 64 pieces: the caller concatenates


@pytest.mark.gpu
def test_conv3_wgrad_band_pieces_on_4x4_maps():
    """The pieces form on 4 x 4 maps (sixteen per item: pieces of a multiple of 16 maps) == the concatenated batch, bit for bit; other piece
    sizes are refused (the caller concatenates)."""
    from spatiotemporal_variable_separation_amd import ops
    dtype = torch.bfloat16
    pairs = [(_rand((32, 96, 4, 4), 500 + i).to(dtype).cuda(), _rand((32, 64, 4, 4), 600 + i).to(dtype).cuda()) for i in range(3)]
    shape = (96, 64, 3, 3)
    dz, x = torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])
    want = ops.conv_wgrad(dz, x, shape, 1, 1, False)
    got = ops.conv3_wgrad_band_pieces(pairs, shape)
    torch.cuda.synchronize()
    assert got is not None and torch.equal(got, want)
    odd = [(p[0][:8].contiguous(), p[1][:8].contiguous()) for p in pairs]
    assert ops.conv3_wgrad_band_pieces(odd, shape) is None


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('geom', [
    (6, 64, 32, 32, 128),     # DCGAN encoder layer 2 (nf = 64): planes [6, 256, 16, 16]
    (5, 128, 16, 16, 256),    # layer 3: planes [5, 512, 8, 8] (8 x 8 maps, four per workgroup; 5 = one full group + 1)
    (3, 16, 64, 64, 40),      # planes [3, 64, 32, 32]: one 64-channel phase, ragged output-channel tile
    (2, 32, 128, 128, 32),    # planes [2, 128, 64, 64]
    (37, 256, 8, 8, 512),     # DCGAN encoder layer 4 / decoder layer 1 (conv.py:122, 260): planes [37, 1024, 4, 4], sixteen maps per item
    (16, 64, 8, 8, 40),       # 4 x 4 planes, ragged output-channel tile
])
def test_conv_k4s2_on_parity_planes_matches_fp64(dtype, geom):
    """The k4 s2 p1 family without a column matrix (csrc/vs_conv_k4s2.hip: parity planes + row-band kernels) against fp64 torch on the
    same 16-bit operands: Conv2d forward and weight gradient, ConvTranspose2d input gradient and weight gradient."""
    from spatiotemporal_variable_separation_amd import ops
    B, C, H, W, M = geom
    x = _rand((B, C, H, W), 301).to(dtype)
    assert ops.conv_k4s2_supported(x.cuda(), M)
    planes = ops.space_to_depth2(x.cuda())
    # planes: channel (py * 2 + px) * C + c = x[c][2 y + py][2 x + px]
    want = torch.stack([x[:, :, py::2, px::2] for py in (0, 1) for px in (0, 1)], dim=1).reshape(B, 4 * C, H // 2, W // 2)
    assert torch.equal(planes.cpu(), want)
    # Conv2d(C, M, 4, 2, 1): forward + weight gradient
    w = _rand((M, C, 4, 4), 302, 0.3).to(dtype)
    bias = _rand((M,), 303)
    wp = ops.conv_k4s2_pack_weight(w.float().cuda(), dtype)
    y = ops.conv_k4s2_gather(planes, wp, bias.cuda(), M, torch.float32)
    w64 = w.double().requires_grad_(True)
    ref = F.conv2d(x.double(), w64, bias.double(), stride=2, padding=1)
    assert ((y.cpu().double() - ref.detach()).abs().max() / ref.detach().abs().max()).item() < 1e-5
    dz = _rand(tuple(ref.shape), 304).to(dtype)
    ref.backward(dz.double())
    dw = ops.conv_k4s2_wgrad(dz.cuda(), planes, (M, C, 4, 4))
    pend = _rand((M, C, 4, 4), 305).cuda()
    acc = ops.conv_k4s2_wgrad(dz.cuda(), planes, (M, C, 4, 4), into=pend.clone())
    torch.cuda.synchronize()
    scale = w64.grad.abs().max()
    assert ((dw.cpu().double() - w64.grad).abs().max() / scale).item() < 2e-6
    assert ((acc.cpu().double() - (w64.grad + pend.cpu().double())).abs().max() / scale).item() < 2e-6
    # ConvTranspose2d(M, C, 4, 2, 1) with output gradient x [B, C, H, W]: input gradient [B, M, H/2, W/2] and weight gradient [M, C, 4, 4]
    wt = _rand((M, C, 4, 4), 306, 0.3).to(dtype)
    inp = _rand((B, M, H // 2, W // 2), 307).to(dtype)
    i64, wt64 = inp.double().requires_grad_(True), wt.double().requires_grad_(True)
    F.conv_transpose2d(i64, wt64, None, stride=2, padding=1).backward(x.double())
    dx = ops.conv_k4s2_gather(planes, ops.conv_k4s2_pack_weight(wt.float().cuda(), dtype), None, M, torch.float32, role='dgrad')
    dwt = ops.conv_k4s2_wgrad(inp.cuda(), planes, (M, C, 4, 4))
    torch.cuda.synchronize()
    assert ((dx.cpu().double() - i64.grad).abs().max() / i64.grad.abs().max()).item() < 1e-5
    assert ((dwt.cpu().double() - wt64.grad).abs().max() / wt64.grad.abs().max()).item() < 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_conv3_pack_weights_in_one_launch_equals_single_packs(dtype):
    """vs_conv3_img16_pack_weights (all the stale pre-packs of a step in one launch) == vs_conv3_img16_pack_weight job by job, bit for bit,
    forward and flipped, ragged row tiles included."""
    from spatiotemporal_variable_separation_amd import ops
    shapes = [(64, 64), (40, 128), (196, 256), (512, 64), (33, 16), (128, 192)]
    ws = [_rand((co, ci, 3, 3), 400 + i, 0.3).cuda() for i, (co, ci) in enumerate(shapes)]
    jobs, want = [], []
    for w in ws:
        for flip in (False, True):
            K = w.shape[0] if flip else w.shape[1]
            if K % 16:
                continue
            jobs.append((w, flip, None))
            want.append(ops.conv3_img16_pack_weight(w, dtype, flip))
    got = ops.conv3_img16_pack_weights(jobs, dtype)
    torch.cuda.synchronize()
    assert len(got) == len(want) >= 9
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


THIN_GEOMS = [
    # (B, Cin, H, W, Cout, k, stride, pad, transposed)
    (3, 5, 64, 64, 64, 4, 2, 1, False),     # DCGAN encoder c1 at width (conv.py:119): forward = expand (5 thin channels), weight gradient
    (2, 8, 32, 32, 64, 3, 1, 1, False),     # VGG encoder first layer on 8 stacked frames (conv.py:130)
    (2, 4, 64, 64, 64, 3, 1, 1, False),     # SST encoder first layer (conv.py:345)
    (3, 1, 64, 32, 32, 4, 2, 1, False),     # one thin channel, rows of 16 pixels
    (3, 64, 32, 32, 1, 4, 2, 1, True),      # DCGAN decoder upc5 (conv.py:264): forward = reduce over four output parities
    (2, 64, 32, 32, 2, 3, 1, 1, True),      # VGG decoder last layer (conv.py:300)
    (2, 64, 64, 64, 1, 3, 1, 1, False),     # SST decoder last layer (conv.py:420): Conv2d seen from its output (flipped taps)
    (2, 32, 16, 32, 3, 3, 1, 1, False),     # three thin channels (a masked fourth), rows of 32 on 16 x 32 maps
    (2, 64, 8, 64, 2, 4, 2, 1, True),       # k4 s2 with two thin channels
    (5, 96, 16, 32, 3, 3, 1, 1, True),      # 96 channels, an odd batch
]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('geom', THIN_GEOMS)
def test_conv_thin_kernels_match_fp64(dtype, geom):
    """The first / last layers (1..8 channels on the image side) through csrc/vs_conv_thin.hip -- expand, reduce and the weight gradient --
    against fp64 on the same 16-bit operands; the dispatch inside ops.conv_fwd / conv_dgrad / conv_wgrad must pick them."""
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd._lib import dtype_code
    B, Cin, H, W, Cout, k, s, p, tr = geom
    x = _rand((B, Cin, H, W), 41).to(dtype)
    wshape = (Cin, Cout, k, k) if tr else (Cout, Cin, k, k)
    w = _rand(wshape, 42, 0.3).to(dtype)
    bias = _rand((Cout,), 43)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    fn = F.conv_transpose2d if tr else F.conv2d
    y64 = fn(x64, w64, bias.double(), stride=s, padding=p)
    OH, OW = y64.shape[2], y64.shape[3]
    dy = _rand(tuple(y64.shape), 44).to(dtype)
    y64.backward(dy.double())
    code = dtype_code(x.cuda())
    plans = {op: ops._thin_plan(op, code, B, Cin, H, W, Cout, OH, OW, k, s, p, tr, wgrad_max_m=8) for op in ('fwd', 'dgrad', 'wgrad')}
    assert plans['fwd'] is not None and plans['wgrad'] is not None, plans
    if Cout <= 8:
        assert plans['dgrad'] is not None, plans

    def rel(a, b):
        return ((a.cpu().double() - b).norm() / (b.norm() + 1e-30)).item()
    y = ops.conv_fwd(x.cuda(), w.cuda(), bias.cuda(), s, p, tr, torch.float32)
    assert tuple(y.shape) == tuple(y64.shape)
    assert rel(y, y64.detach()) < 1e-5, f'fwd {geom} {dtype}'
    y16 = ops.conv_fwd(x.cuda(), w.cuda(), bias.cuda(), s, p, tr, dtype)
    assert torch.equal(y16.cpu(), y.cpu().to(dtype)), 'typed store = rounding of the fp32 result'
    # (the dispatch in ops.conv_wgrad takes the thin kernel up to two thin channels; the kernel itself serves up to eight)
    big, small = (dy.cuda(), x.cuda()) if plans['wgrad'][0] == 'wgrad_big_dy' else (x.cuda(), dy.cuda())
    dw = ops.conv_thin_wgrad(big, small, wshape, k, s, *plans['wgrad'][5:])
    assert rel(dw, w64.grad) < 1e-5, f'wgrad {geom} {dtype}'
    base = _rand(wshape, 45).cuda()
    acc = base.clone()
    ops.conv_thin_wgrad(big, small, wshape, k, s, *plans['wgrad'][5:], into=acc)
    assert rel(acc, base.cpu().double() + w64.grad) < 1e-5, 'accumulating form'
    dw2 = ops.conv_thin_wgrad(big, small, wshape, k, s, *plans['wgrad'][5:])
    assert torch.equal(dw, dw2), 'fixed summation order: bit-reproducible'
    assert rel(ops.conv_wgrad(dy.cuda(), x.cuda(), wshape, s, p, tr), w64.grad) < 1e-5, 'through the dispatch'
    dx = ops.conv_dgrad(dy.cuda(), w.cuda(), x.shape, s, p, tr, torch.float32, cols_from_wgrad=tr)
    assert rel(dx, x64.grad) < 1e-5, f'dgrad {geom} {dtype}'
    if plans['dgrad'] is not None:
        dx16 = ops.conv_dgrad(dy.cuda(), w.cuda(), x.shape, s, p, tr, dtype)
        assert torch.equal(dx16.cpu(), dx.cpu().to(dtype))


# (geometry, the 16-bit kernel family that serves conv_fwd / conv_dgrad / conv_wgrad under VARSEP_FP32_SPLIT=1, as ops.profile_collect names it;
# None: no split route serves that op there and the fp32 column-matrix route keeps it).  The smallest shapes that reach each family; the routes
# are those tests/golden/conv_ops_routes.json records for these shapes.
SPLIT_GEOMS = [
    ((2, 64, 32, 32, 96, 3, 1, 1, False), ('vs_conv3_band:fwd', 'vs_conv3_band:dgrad', 'vs_conv3_wgrad_band')),
    ((8, 64, 16, 16, 33, 3, 1, 1, False), ('vs_conv3_img16:fwd', 'vs_conv3_band:dgrad', 'vs_conv3_wgrad_band')),      # few maps: split slabs + slab sum
    ((16, 64, 32, 32, 64, 4, 2, 1, False), ('vs_conv_k4s2:fwd', 'vs_convT_tap:dgrad', 'vs_conv_k4s2:wgrad')),
    ((16, 64, 16, 16, 64, 4, 2, 1, True), ('vs_convT_tap:fwd', 'vs_conv_k4s2:dgrad', 'vs_conv_k4s2:wgrad')),
    ((3, 5, 64, 64, 64, 4, 2, 1, False), ('vs_conv_thin:fwd', None, 'vs_conv_thin:wgrad')),
    ((3, 64, 32, 32, 1, 4, 2, 1, True), ('vs_conv_thin:fwd', 'vs_conv_thin:dgrad', 'vs_conv_thin:wgrad')),
    ((2, 64, 64, 64, 1, 3, 1, 1, False), ('vs_conv_thin:fwd', 'vs_conv_thin:dgrad', 'vs_conv_thin:wgrad')),
]


@pytest.mark.gpu
@pytest.mark.parametrize('geom,families', SPLIT_GEOMS)
def test_fp32_split_conv_ops_match_fp64(geom, families, monkeypatch):
    """VARSEP_FP32_SPLIT=1 op by op: fp32 conv_fwd (with bias), conv_dgrad, conv_wgrad fresh and accumulated into a pending gradient through six
    launches of a 16-bit kernel family, each against fp64 within the fp32 bound of this file (relative L2 < 1e-5), and that the six launches
    ran and no column matrix was built."""
    from spatiotemporal_variable_separation_amd import ops
    monkeypatch.setenv('VARSEP_FP32_SPLIT', '1')
    B, Cin, H, W, Cout, k, s, p, tr = geom
    x = _rand((B, Cin, H, W), 1)
    wshape = (Cin, Cout, k, k) if tr else (Cout, Cin, k, k)
    w = _rand(wshape, 2, 0.3)
    bias = _rand((Cout,), 3)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = (F.conv_transpose2d if tr else F.conv2d)(x64, w64, bias.double(), stride=s, padding=p)
    dy = _rand(tuple(y64.shape), 4)
    y64.backward(dy.double())
    g0 = _rand(wshape, 5)

    def rel(a, b):
        return ((a.cpu().double() - b).norm() / (b.norm() + 1e-30)).item()

    def launches(call):
        ops.profile_reset(True)
        r = call()
        return r, ops.profile_collect()
    xc, wc, dyc = x.cuda(), w.cuda(), dy.cuda()
    acc = g0.clone().cuda()
    runs = (('fwd', families[0], lambda: ops.conv_fwd(xc, wc, bias.cuda(), s, p, tr, torch.float32), lambda r: rel(r, y64.detach())),
            ('dgrad', families[1], lambda: ops.conv_dgrad(dyc, wc, x.shape, s, p, tr, torch.float32), lambda r: rel(r, x64.grad)),
            ('wgrad', families[2], lambda: ops.conv_wgrad(dyc, xc, wshape, s, p, tr), lambda r: rel(r, w64.grad)),
            ('wgrad into', families[2], lambda: ops.conv_wgrad(dyc, xc, wshape, s, p, tr, into=acc), lambda r: rel(r.cpu().double() - g0.double(), w64.grad)))
    for what, family, call, error in runs:
        r, prof = launches(call)
        err = error(r)
        print('%s %s: relative L2 %.2e, launches %s' % (geom, what, err, {n: v['n'] for n, v in prof.items()}))
        assert err < 1e-5, f'{what} {geom}: {err:.3e}'
        if family is not None:
            assert prof.get(family + '<bf16>', {}).get('n') == 6, (what, geom, sorted(prof))
            assert not [n for n in prof if n.startswith('vs_conv') and '_cols:' in n], (what, geom, sorted(prof))
    assert acc.data_ptr() == r.data_ptr()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('shape,groups', [((200, 64, 8, 8), 2), ((24, 512, 4, 4), 8), ((6, 40, 16, 16), 3)])
def test_batchnorm_small_one_launch_with_call_groups_equals_one_call_per_group(dtype, shape, groups, monkeypatch):
    """vs_bn_train_fwd_small_groups (several reference calls stacked along the batch axis, per-call statistics, running estimates folded in call
    order) == the one-call launch applied to each group in turn, bit for bit (the VGG / DCGAN encoders' paired calls, the decoders'
    per-frame calls, conv.py:41-60)."""
    from spatiotemporal_variable_separation_amd import ops
    monkeypatch.setenv('VS_BN_SMALL_GROUPS', '1')          # (not the default route: see ops.bn_small_supported)
    B, C, H, W = shape
    x = (_rand(shape, 71) * 3 + 0.5).to(dtype).cuda()
    gamma, beta = (_rand((C,), 72) + 1.5).cuda(), _rand((C,), 73).cuda()
    assert ops.bn_small_supported(x, groups)
    rm, rv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
    y, mean, invstd = ops.bn_train_fwd_small(x, gamma, beta, 'leaky_relu', dtype, rm, rv, 0.1, 1e-5, groups=groups)
    rm1, rv1 = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
    Bg = B // groups
    for g in range(groups):
        yg, mg, ig = ops.bn_train_fwd_small(x[g * Bg:(g + 1) * Bg].contiguous(), gamma, beta, 'leaky_relu', dtype, rm1, rv1, 0.1, 1e-5)
        assert torch.equal(y[g * Bg:(g + 1) * Bg], yg) and torch.equal(mean[g], mg[0]) and torch.equal(invstd[g], ig[0])
    assert torch.allclose(rm, rm1, rtol=1e-6, atol=1e-7) and torch.allclose(rv, rv1, rtol=1e-6, atol=1e-7)
    # and against the two-launch path on the stacked tensor
    rm2, rv2 = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
    m2, i2 = ops.bn_stats(x, rm2, rv2, 0.1, 1e-5, groups=groups)
    y2 = ops.bn_act_fwd(x, m2, i2, gamma, beta, 'leaky_relu', dtype, groups=groups)
    assert torch.allclose(mean, m2, rtol=1e-5, atol=1e-6) and torch.allclose(invstd, i2, rtol=1e-5, atol=1e-6)
    assert (y.float() - y2.float()).abs().max().item() <= (2e-2 if dtype != torch.float32 else 1e-5) * y2.float().abs().max().item()
    assert torch.allclose(rm, rm2, rtol=1e-5, atol=1e-6) and torch.allclose(rv, rv2, rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('geom,groups', [((6, 64, 32, 32, 40), 2), ((12, 128, 8, 8, 64), 3), ((4, 64, 64, 64, 32), 1), ((9, 64, 16, 16, 96), 9)])
def test_conv3_band_leaves_batchnorm_sums_of_its_stored_output(dtype, geom, groups, monkeypatch):
    """vs_conv3_band_bn: (sum, sum of squares) per (call group, channel) of the values AS STORED, added to a persistent buffer in the epilogue;
    vs_bn_stats_from_sums_fold = vs_bn_stats on the stored tensor (mean / invstd per group, running estimates folded in call order) and
    leaves the buffer at zero."""
    from spatiotemporal_variable_separation_amd import ops
    monkeypatch.setenv('VS_BAND_BN_SUMS', '1')            # (an opt-in route: see ops.conv_band_bn_supported)
    B, Cin, H, W, Cout = geom
    x = _rand((B, Cin, H, W), 81).to(dtype).cuda()
    w = _rand((Cout, Cin, 3, 3), 82, 0.3)
    bias = _rand((Cout,), 83).cuda()
    assert ops.conv_band_bn_supported(B, Cin, H, W, Cout, groups, dtype)
    wp = ops.conv3_img16_pack_weight(w.cuda(), dtype, False)
    sums = ops.bn_sums_buffer('test-%s-%s' % (geom, dtype), groups, Cout, x.device)
    assert float(sums.abs().sum()) == 0.0
    y = ops.conv3_band(x, wp, bias, Cout, dtype, bn_sums=sums, groups=groups)
    y_plain = ops.conv3_band(x, wp, bias, Cout, dtype)
    assert torch.equal(y, y_plain)
    yg = y.double().view(groups, B // groups, Cout, H * W)
    ref = torch.stack([yg.sum(dim=(1, 3)), (yg * yg).sum(dim=(1, 3))], dim=-1)
    assert ((sums - ref).abs().max() / ref.abs().max()).item() < 1e-6
    rm, rv = torch.zeros(Cout, device='cuda'), torch.ones(Cout, device='cuda')
    mean, invstd = ops.bn_stats_from_sums_fold(sums, (B // groups) * H * W, rm, rv, 0.1, 1e-5)
    assert float(sums.abs().sum()) == 0.0, 'left at zero for the next step'
    rm2, rv2 = torch.zeros(Cout, device='cuda'), torch.ones(Cout, device='cuda')
    m2, i2 = ops.bn_stats(y, rm2, rv2, 0.1, 1e-5, groups=groups)
    assert torch.allclose(mean, m2, rtol=1e-5, atol=1e-6) and torch.allclose(invstd, i2, rtol=1e-5, atol=1e-6)
    assert torch.allclose(rm, rm2, rtol=1e-5, atol=1e-6) and torch.allclose(rv, rv2, rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('geom,groups', [((6, 64, 32, 32, 40), 2), ((12, 128, 8, 8, 64), 3), ((4, 64, 64, 64, 32), 1), ((9, 64, 16, 16, 96), 9),
                                         ((200, 16, 16, 16, 72), 2)])
def test_conv3_band_partial_sum_table_gives_the_batchnorm_statistics(dtype, geom, groups, monkeypatch):
    """vs_conv3_band_bn_parts (round 4; opt-in, VS_BAND_BN_SUMS=parts: measured slower than the statistics pass it replaces): every workgroup writes the (sum, sum of squares)
    of its 32 channels x 256 stored values to its own table row, no atomics; the table's column sums are the sums of the stored tensor, the
    output equals the plain kernel's, vs_bn_stats_from_parts_fold == vs_bn_stats on the stored tensor (mean / invstd per call group, running
    estimates folded in call order), launch-to-launch bit-reproducible."""
    from spatiotemporal_variable_separation_amd import ops
    monkeypatch.setenv('VS_BAND_BN_SUMS', 'parts')
    B, Cin, H, W, Cout = geom
    x = _rand((B, Cin, H, W), 81).to(dtype).cuda()
    w = _rand((Cout, Cin, 3, 3), 82, 0.3)
    bias = _rand((Cout,), 83).cuda()
    assert ops.band_bn_mode() == 'parts' and ops.conv_band_bn_supported(B, Cin, H, W, Cout, groups, dtype)
    wp = ops.conv3_img16_pack_weight(w.cuda(), dtype, False)
    y, parts = ops.conv3_band_parts(x, wp, bias, Cout, dtype)
    y2, parts2 = ops.conv3_band_parts(x, wp, bias, Cout, dtype)
    assert torch.equal(y, ops.conv3_band(x, wp, bias, Cout, dtype)) and torch.equal(parts, parts2)
    rows = parts.shape[0]
    assert rows % groups == 0
    yg = y.double().view(groups, B // groups, Cout, H * W)
    ref = torch.stack([yg.sum(dim=(1, 3)), (yg * yg).sum(dim=(1, 3))], dim=-1)
    got = parts.double().view(groups, rows // groups, Cout, 2).sum(dim=1)
    assert ((got - ref).abs().max() / ref.abs().max()).item() < 1e-6
    rm, rv = torch.zeros(Cout, device='cuda'), torch.ones(Cout, device='cuda')
    mean, invstd = ops.bn_stats_from_parts_fold(parts, groups, (B // groups) * H * W, rm, rv, 0.1, 1e-5)
    rm2, rv2 = torch.zeros(Cout, device='cuda'), torch.ones(Cout, device='cuda')
    m2, i2 = ops.bn_stats(y, rm2, rv2, 0.1, 1e-5, groups=groups)
    assert torch.allclose(mean, m2, rtol=1e-5, atol=1e-6) and torch.allclose(invstd, i2, rtol=1e-5, atol=1e-6)
    assert torch.allclose(rm, rm2, rtol=1e-5, atol=1e-6) and torch.allclose(rv, rv2, rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_conv_k4s2_planes_partial_sum_table(dtype):
    """The same table from the k4 s2 p1 gather on parity planes (the DCGAN encoder's conv -> BatchNorm layers, conv.py:119-122)."""
    from spatiotemporal_variable_separation_amd import ops
    B, C, H, W, M, groups = 6, 64, 32, 32, 128, 2
    x = _rand((B, C, H, W), 91).to(dtype).cuda()
    planes = ops.space_to_depth2(x)
    w = _rand((M, C, 4, 4), 92, 0.3)
    bias = _rand((M,), 93).cuda()
    wp = ops.conv_k4s2_pack_weight(w.cuda(), dtype)
    y, parts = ops.conv3_band_parts(planes, wp, bias, M, dtype, k4=True)
    assert torch.equal(y, ops.conv_k4s2_gather(planes, wp, bias, M, dtype))
    yg = y.double().view(groups, B // groups, M, (H // 2) * (W // 2))
    ref = torch.stack([yg.sum(dim=(1, 3)), (yg * yg).sum(dim=(1, 3))], dim=-1)
    got = parts.double().view(groups, parts.shape[0] // groups, M, 2).sum(dim=1)
    assert ((got - ref).abs().max() / ref.abs().max()).item() < 1e-6
    mean, invstd = ops.bn_stats_from_parts_fold(parts, groups, (B // groups) * (H // 2) * (W // 2))
    m2, i2 = ops.bn_stats(y, None, None, 0.1, 1e-5, groups=groups)
    assert torch.allclose(mean, m2, rtol=1e-5, atol=1e-6) and torch.allclose(invstd, i2, rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('geom', [(21, 64, 8, 8, 96), (256, 256, 8, 8, 512)])
def test_conv_k4s2_gather_on_4x4_planes_matches_fp64(dtype, geom):
    """8 x 8 maps (the DCGAN encoder's c4, conv.py:122): parity planes of 4 x 4 pixels (8-byte rows) and the gather on them (sixteen maps per
    workgroup of the row-band kernel); since round 4 the weight gradient of such a layer runs on the planes as well
    (test_conv_k4s2_on_parity_planes_matches_fp64 has the 4 x 4 plane geometries)."""
    from spatiotemporal_variable_separation_amd import ops
    B, C, H, W, M = geom
    x = _rand((B, C, H, W), 311).to(dtype)
    assert ops.conv_k4s2_gather_supported(x.cuda(), M) and ops.conv_k4s2_supported(x.cuda(), M)
    planes = ops.space_to_depth2(x.cuda())
    want = torch.stack([x[:, :, py::2, px::2] for py in (0, 1) for px in (0, 1)], dim=1).reshape(B, 4 * C, H // 2, W // 2)
    assert torch.equal(planes.cpu(), want)
    w = _rand((M, C, 4, 4), 312, 0.3).to(dtype)
    bias = _rand((M,), 313)
    y = ops.conv_k4s2_gather(planes, ops.conv_k4s2_pack_weight(w.float().cuda(), dtype), bias.cuda(), M, torch.float32)
    ref = F.conv2d(x.double(), w.double(), bias.double(), stride=2, padding=1)
    assert ((y.cpu().double() - ref).abs().max() / ref.abs().max()).item() < 1e-5


@pytest.mark.parametrize('shape', [(8, 96, 16, 16, 4), (32, 64, 16, 16, 2), (48, 128, 32, 32, 3), (200, 64, 32, 32, 2), (6, 520, 8, 8, 3)])
def test_bn_group_sums_inside_the_backward_launch_equal_the_separate_launch(shape, monkeypatch):
    """vs_bn_act_bwd_gsum: the sums of d gamma / d beta over the call groups are formed by the LAST workgroup of each channel to arrive inside
    the one-launch backward kernels (small / resident / resident + LDS slabs: csrc/vs_norm.hip, bn_group_sums_arrive) instead of a launch of
    their own.  Same group order, so BIT-equal to the separate launch (VS_BN_GSUM_FUSED=0), on every one of 30 back-to-back calls beside a
    bandwidth-hungry kernel on another stream (a stale partial or a lost arrival would show as a wrong or missing sum)."""
    from spatiotemporal_variable_separation_amd import ops
    from oracle.detdata import det_uniform
    B, C, H, W, G = shape
    x = ((det_uniform((B, C, H, W), 71) - 0.5) * 2).to(torch.bfloat16).cuda()
    dy = ((det_uniform((B, C, H, W), 73) - 0.5) * 2).to(torch.bfloat16).cuda()
    gamma = (det_uniform((C,), 75) + 0.5).cuda()
    beta = (det_uniform((C,), 77) - 0.5).cuda()
    mean, invstd = ops.bn_stats(x, None, None, 0.1, 1e-5, groups=G)
    monkeypatch.setenv('VS_BN_GSUM_FUSED', '0')
    dx0, dg0, db0 = ops.bn_act_bwd(dy, x, mean, invstd, gamma, beta, 'leaky_relu', True, torch.bfloat16, groups=G)
    torch.cuda.synchronize()
    monkeypatch.setenv('VS_BN_GSUM_FUSED', '1')
    noise = torch.empty(32 << 20, device='cuda')
    side = torch.cuda.Stream()
    for it in range(30):
        if it % 3 == 0:
            with torch.cuda.stream(side):
                noise.add_(1.0)
        dx1, dg1, db1 = ops.bn_act_bwd(dy, x, mean, invstd, gamma, beta, 'leaky_relu', True, torch.bfloat16, groups=G)
        assert torch.equal(dg1, dg0) and torch.equal(db1, db0), f'{shape} call {it}: group sums differ: {(dg1 - dg0).abs().max().item()}'
        assert torch.equal(dx1, dx0)
    torch.cuda.synchronize()


# ---- entry points the model runs that had no direct test: ops.chan_sum, ops.bn_stats_ub + ops.bn_act_fwd(running=...), ops.bn_act_bwd(training=False)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('shape', [(3, 5, 7, 7), (2, 1, 64, 64), (64, 3, 33, 33)])
def test_chan_sum_matches_fp64_and_is_bitwise_repeatable(dtype, shape):
    """The bias gradient of every convolution without BatchNorm (vs_chan_sum_ws): per-chunk fp64 partial sums in a workspace, finished in a
    fixed order -- one channel (all chunks meet on one address) included.  2e-6 relative L2: this file's bound for fp32 results of
    fp64-accumulated reductions."""
    from spatiotemporal_variable_separation_amd import ops
    x = _rand(shape, 21).to(dtype).cuda()
    ref = x.double().sum((0, 2, 3))
    out = ops.chan_sum(x)
    assert out.dtype == torch.float32 and tuple(out.shape) == (shape[1],)
    err = ((out.double() - ref).norm() / ref.norm()).item()
    assert err < 2e-6, (shape, dtype, err)
    assert torch.equal(ops.chan_sum(x), out)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('groups', [1, 3])
def test_batchnorm_running_estimates_folded_by_the_apply_launch(dtype, groups):
    """ops.bn_stats_ub + ops.bn_act_fwd(..., running=(ub, rm, rv, momentum)): the route functional._bn_apply takes in training with tracked
    running estimates when no one-launch form serves the tensor.  Against `groups` sequential fp64 BatchNorm2d calls: y and the running
    estimates after 1 and after 16 calls (bounds of test_batchnorm_act_fwd_bwd), and bit-equal to bn_stats(..., rm, rv) + bn_act_fwd."""
    from spatiotemporal_variable_separation_amd import ops
    B, C, H, W = 6, 7, 12, 10
    x = (_rand((B, C, H, W), 22) * 2 + 0.3).to(dtype)
    gamma, beta = 1 + _rand((C,), 23, 0.3), _rand((C,), 24, 0.2)
    rm, rv = _rand((C,), 25, 0.1), 1 + _rand((C,), 26, 0.2)
    xc, gc, bc = x.cuda(), gamma.cuda(), beta.cuda()
    assert not ops.bn_small_supported(xc, groups) and not ops.bn_slab_supported(xc, groups)       # so this IS the route _bn_apply takes
    bn = torch.nn.BatchNorm2d(C).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    Bg = B // groups

    def reference_call():
        with torch.no_grad():
            return torch.cat([F.leaky_relu(bn(x[g * Bg:(g + 1) * Bg].double()), 0.2) for g in range(groups)])

    def rel(a, b):
        return ((a.cpu().double() - b).norm() / (b.norm() + 1e-30)).item()
    y64 = reference_call()
    rmc, rvc = rm.clone().cuda(), rv.clone().cuda()
    mean, invstd, ub = ops.bn_stats_ub(xc, 1e-5, groups=groups)
    y = ops.bn_act_fwd(xc, mean, invstd, gc, bc, 'leaky_relu', torch.float32, groups=groups, running=(ub, rmc, rvc, 0.1))
    assert tuple(mean.shape) == tuple(invstd.shape) == tuple(ub.shape) == (groups, C)
    assert rel(y, y64) < 2e-6
    assert rel(rmc, bn.running_mean) < 2e-6 and rel(rvc, bn.running_var) < 2e-6
    # the two-launch statistics + the plain apply: same kernels, same arithmetic
    rm2, rv2 = rm.clone().cuda(), rv.clone().cuda()
    mean2, invstd2 = ops.bn_stats(xc, rm2, rv2, 0.1, 1e-5, groups=groups)
    y2 = ops.bn_act_fwd(xc, mean2, invstd2, gc, bc, 'leaky_relu', torch.float32, groups=groups)
    assert torch.equal(mean, mean2) and torch.equal(invstd, invstd2)
    assert torch.equal(y, y2) and torch.equal(rmc, rm2) and torch.equal(rvc, rv2)
    for _ in range(15):
        reference_call()
        ops.bn_act_fwd(xc, mean, invstd, gc, bc, 'leaky_relu', torch.float32, groups=groups, running=(ub, rmc, rvc, 0.1))
        ops.bn_stats(xc, rm2, rv2, 0.1, 1e-5, groups=groups)
    assert rel(rmc, bn.running_mean) < 1e-5 and rel(rvc, bn.running_var) < 1e-5
    assert torch.equal(rmc, rm2) and torch.equal(rvc, rv2)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('act', ['leaky_relu', 'none', 'sigmoid'])
@pytest.mark.parametrize('shape', [(5, 7, 12, 10), (3, 5, 9, 9)])
@pytest.mark.parametrize('groups', [1, 2])
def test_batchnorm_act_bwd_eval_mode(groups, shape, act, dtype):
    """ops.bn_act_bwd(..., training=False): the statistics are constants (mean = running_mean, invstd = 1 / sqrt(running_var + eps)).  Against
    fp64 eval-mode batch_norm + activation; `groups` calls of `shape` stacked along the batch axis, each with running statistics of its own,
    the parameter gradients summed over the calls.  Bounds of the training-mode test (test_batchnorm_act_fwd_bwd)."""
    from spatiotemporal_variable_separation_amd import ops
    Bg, C, H, W = shape
    x = (_rand((groups * Bg, C, H, W), 27) * 2 + 0.3).to(dtype)
    dy = _rand((groups * Bg, C, H, W), 28)
    gamma, beta = 1 + _rand((C,), 29, 0.3), _rand((C,), 30, 0.2)
    rm, rv = _rand((groups, C), 31, 0.4), 1 + _rand((groups, C), 32, 0.5)
    eps = 1e-5
    acts = {'leaky_relu': lambda t: F.leaky_relu(t, 0.2), 'none': lambda t: t, 'sigmoid': torch.sigmoid}
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y64 = torch.cat([acts[act](F.batch_norm(x64[g * Bg:(g + 1) * Bg], rm[g].double(), rv[g].double(), g64, b64, False, 0.1, eps)) for g in range(groups)])
    y64.backward(dy.double())
    mean, invstd = rm.cuda(), torch.rsqrt(rv.double() + eps).float().cuda()
    xc = x.cuda()
    y = ops.bn_act_fwd(xc, mean, invstd, gamma.cuda(), beta.cuda(), act, torch.float32, groups=groups)
    dx, dg, db = ops.bn_act_bwd(dy.cuda(), xc, mean, invstd, gamma.cuda(), beta.cuda(), act, False, torch.float32, groups=groups)

    def rel(a, b):
        return ((a.cpu().double() - b).norm() / (b.norm() + 1e-30)).item()
    assert rel(y, y64.detach()) < 2e-6
    assert rel(dx, x64.grad) < 2e-5
    assert tuple(dg.shape) == tuple(db.shape) == (C,)
    assert rel(dg, g64.grad) < 2e-5 and rel(db, b64.grad) < 2e-5

"""Nothing writes outside its output, and every element of an output is written: each `ops` wrapper runs twice, plain and with every tensor it
allocates between two 4096-byte bands of 0xFF (tests/guard_util.py).  The pad keeps the alignment class of a plain allocation, so the guarded
call takes the same code path: the two results are bit-equal (where an existing test calls a result order-dependent, that test's bound),
the guard bytes are intact and the guarded result holds no NaN -- an element that was never written would still be 0xFF.  The fp64 correctness
of the plain call is the business of the other test files and is not restated here.

The second half drives every entry point with pointers OFF 16-byte alignment (inputs: `embed(t, offset=1)`, outputs:
`guarded_ops(misalign=1)`) from ONE table, MISALIGNED, that states per entry point what its host code does with such a pointer (read, not
discovered at run time): 'ok' -- it selects an element-wise form and gives the aligned call's values to that call's existing bound -- or
'refused' -- a VarsepHipError that names the entry point, and nothing launched.

Out of reach: a stray write farther than 4096 bytes from an output, and any out-of-range read.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = (F32, BF16, F16)


def _rand(shape, salt, scale=1.0, dtype=F32):
    from oracle.detdata import det_uniform
    return ((det_uniform(tuple(shape), salt) - 0.5) * 2.0 * scale).to(dtype).cuda()


def _flat(res):
    out = []
    for r in (res if isinstance(res, (tuple, list)) else (res,)):
        if isinstance(r, (tuple, list)):
            out += _flat(r)
        elif r is not None:
            out.append(r)
    return out


def _twice(fn, what, loose=None, misalign=0):
    """fn(): one wrapper call on fixed inputs -> its outputs.  `loose`: {output index: (rtol, atol)} for order-dependent sums."""
    from guard_util import guarded_ops
    plain = _flat(fn())
    with pytest.MonkeyPatch.context() as mp:
        allocs = guarded_ops(mp, misalign=misalign)
        guarded = _flat(fn())
        torch.cuda.synchronize()
    assert allocs.guards, (what, 'the wrapper allocated nothing through ops.torch')
    try:
        allocs.check()
    except AssertionError as e:
        raise AssertionError('%s: %s' % (what, e)) from None
    assert len(plain) == len(guarded), what
    for i, (p, g) in enumerate(zip(plain, guarded)):
        assert p.shape == g.shape and p.dtype == g.dtype, (what, i)
        assert not bool(torch.isnan(g.double()).any()), (what, 'output %d holds NaN: an element was never written' % i)
        if loose and i in loose:
            assert torch.allclose(p.double(), g.double(), rtol=loose[i][0], atol=loose[i][1]), (what, i, (p.double() - g.double()).abs().max().item())
        else:
            assert torch.equal(p, g), (what, 'output %d differs from the plain call' % i, (p.double() - g.double()).abs().max().item())
    return plain, guarded, allocs


# ------------------------------------------------------------------------------------------------------------------ element-wise
@pytest.mark.parametrize('n', [1, 3, 1029, 8193])
def test_cast_and_activations_write_n_elements(n):
    from spatiotemporal_variable_separation_amd import ops
    for in_dt in DTYPES:
        x, dy = _rand((n,), 1, 3.0, in_dt), _rand((n,), 2, 3.0, in_dt)
        for out_dt in DTYPES:
            _twice(lambda: ops.cast(x, out_dt), ('cast', n, in_dt, out_dt))
            for act in ('relu', 'sigmoid'):
                y, _, _ = _twice(lambda: ops.act_fwd(x, act, out_dtype=out_dt), ('act_fwd', act, n, in_dt, out_dt))
                _twice(lambda: ops.act_bwd(dy, x, act, out_dtype=out_dt), ('act_bwd', act, n, in_dt, out_dt))


@pytest.mark.parametrize('shape', [(5, 7), (33, 65), (64, 64)])
def test_transpose_cast_writes_its_matrix(shape):
    from spatiotemporal_variable_separation_amd import ops
    for in_dt in DTYPES:
        x = _rand(shape, 3, 1.0, in_dt)
        for out_dt in DTYPES:
            (t,), _, _ = _twice(lambda: ops.transpose_cast(x, out_dt), ('transpose_cast', shape, in_dt, out_dt))
            assert torch.equal(t, x.t().to(out_dt))


@pytest.mark.parametrize('in_dt', DTYPES)
def test_copy2d_and_copy2d_pair_write_their_window_only(in_dt):
    """Strided source (lds = cols + 3), strided destination window (ldd = cols + 5): a copy is exact."""
    from guard_util import embed, window
    from spatiotemporal_variable_separation_amd import ops
    rows = 7
    for cols in (12, 13):                                               # copy2d_pair: 12 = four-element form, 13 = element form
        dense = _rand((2 * rows + 1, cols + 3), 4, 1.0, in_dt)
        src, gs = embed(dense, ld=cols + 3)
        off = torch.tensor([2], dtype=torch.int32, device='cuda')
        for out_dt in DTYPES:
            out, g = window((rows, cols), out_dt, ld=cols + 5, offset=3, device='cuda', rows_before=1)
            ops.copy2d(src, rows, cols, cols + 3, out, cols + 5)
            g.check()
            assert torch.equal(out, dense[:rows, :cols].to(out_dt)), ('copy2d', cols, in_dt, out_dt)
            out, g = window((rows, cols), out_dt, ld=cols + 5, offset=3, device='cuda', rows_before=1)
            ops.copy2d(src, rows, cols, cols + 3, out, cols + 5, col_offset_dev=off, col_offset_scale=1, src_elem_offset=cols + 3)
            g.check()
            assert torch.equal(out, dense[1:rows + 1, 2:cols + 2].to(out_dt)), ('copy2d + device offset', cols, in_dt, out_dt)
            # the pair: rows [0, rows) from a window that moves with the device offset, rows [rows, 2 rows) from a fixed one
            for ldd, woff in ((cols + 4, 4), (cols + 5, 3)):
                wide = _rand((rows + 1, cols + 12), 5, 1.0, in_dt)
                out, g = window((2 * rows, cols), out_dt, ld=ldd, offset=woff, device='cuda', rows_before=1)
                ops.copy2d_pair(wide, rows, cols, cols + 12, out, ldd, off, 4, 0, 4)
                g.check()
                want = torch.cat([wide[:rows, 8:8 + cols], wide[:rows, 4:4 + cols]]).to(out_dt)
                assert torch.equal(out, want), ('copy2d_pair', cols, ldd, in_dt, out_dt)
        gs.check()


@pytest.mark.parametrize('dt', DTYPES)
def test_colsum_and_colsum_multi_write_n_sums(dt):
    from guard_util import embed
    from spatiotemporal_variable_separation_amd import ops
    M = 300                                                             # two row blocks of 256: the sums meet in fp32 atomics
    for N in (130, 7):
        for extra in (8, 1):
            x, _ = embed(_rand((M, N), 6, 1.0, dt), ld=N + extra)
            _twice(lambda: ops.colsum(x, M, N), ('colsum', N, extra, dt), loose={0: (1e-5, 1e-4)})      # (test_colsum_cast_act's bound)
    jobs = [_rand((300, 33), 7, 1.0, F32), _rand((257, 264), 8, 1.0, dt), _rand((5, 7), 9, 1.0, dt), _rand((64, 512), 10, 1.0, dt)[:, 8:136]]
    _twice(lambda: ops.colsum_multi(jobs), ('colsum_multi', dt))


@pytest.mark.parametrize('hw', [(8, 8), (7, 7), (3, 3)])
def test_cat_bcast_writes_its_maps_or_refuses_ragged_planes(hw):
    """HW = 64: one 8-element piece per thread.  HW = 49, 9: vs_cat_bcast_* serve planes of a multiple of 8 elements only and say so."""
    from spatiotemporal_variable_separation_amd import _lib, ops
    B, n, Ca, Cb = 2, 3, 3, 2
    for dt in DTYPES:
        a, x = _rand((B, Ca) + hw, 11, 1.0, dt), _rand((n * B, Cb) + hw, 12, 1.0, dt)
        dout = _rand((n * B, Ca + Cb) + hw, 13, 1.0, dt)
        if hw[0] * hw[1] % 8 == 0:
            for out_dt in (dt, F32):
                _twice(lambda: ops.cat_bcast_fwd(a, x, n, out_dt), ('cat_bcast_fwd', hw, dt, out_dt))
                _twice(lambda: ops.cat_bcast_bwd(dout, B, n, Ca, out_dt, dt), ('cat_bcast_bwd', hw, dt, out_dt))
            _twice(lambda: ops.cat_bcast_bwd(dout, B, n, Ca, dt, dt, need_a=False), ('cat_bcast_bwd dx only', hw, dt))
        else:
            assert not ops.cat_bcast_supported(a, x, n)
            with pytest.raises(_lib.VarsepHipError, match='vs_cat_bcast_fwd'):
                ops.cat_bcast_fwd(a, x, n, dt)
            with pytest.raises(_lib.VarsepHipError, match='vs_cat_bcast_bwd'):
                ops.cat_bcast_bwd(dout, B, n, Ca, dt, dt)


@pytest.mark.parametrize('mixing,Cs,Ct', [('mul', 7, 7), ('concat', 7, 5)])
def test_mix_codes_write_their_codes(mixing, Cs, Ct):
    from spatiotemporal_variable_separation_amd import ops
    B, n = 5, 3
    s, t_rand, t_codes = _rand((B, Cs), 14), _rand((B, Ct), 15), _rand((B, n, Ct), 16)
    for lowp in (None, BF16, F16):
        (z, *_), _, _ = _twice(lambda: ops.mix_codes_fwd(s, t_rand, t_codes, mixing, lowp=lowp), ('mix_codes_fwd', mixing, lowp))
    dz = _rand(tuple(z.shape), 17)
    _twice(lambda: ops.mix_codes_bwd(dz, s, t_rand, t_codes, mixing), ('mix_codes_bwd', mixing))


@pytest.mark.parametrize('out_dt', DTYPES)
def test_slab_sum_writes_its_maps(out_dt):
    from spatiotemporal_variable_separation_amd import ops
    S, B, C, H, W = 3, 2, 5, 16, 16
    slabs, bias = _rand((S, B, C, H, W), 18), _rand((C,), 19)
    a1, a2 = _rand((B, C, H, W), 20), _rand((B, C, H, W), 21)
    _twice(lambda: ops.slab_sum(slabs, bias, out_dt), ('slab_sum', out_dt))
    _twice(lambda: ops.slab_sum(slabs, None, out_dt, addend=a1), ('slab_sum + addend', out_dt))
    _twice(lambda: ops.slab_sum(slabs, bias, out_dt, addend=a1, addend2=a2), ('slab_sum + 2 addends', out_dt))


# ------------------------------------------------------------------------------------------------------------------ BatchNorm
def _bn_inputs(shape, dt, salt=30):
    C = shape[1]
    return (_rand(shape, salt, 2.0, dt), 1 + _rand((C,), salt + 1, 0.3), _rand((C,), salt + 2, 0.2))


@pytest.mark.parametrize('groups', [1, 2])
@pytest.mark.parametrize('hw', [(8, 8), (9, 9), (5, 1)])                # HW 64: 16-byte chunks (vec 1); 81: units per plane (vec 2); 5: elements (vec 0)
def test_batchnorm_two_launch_forms_write_their_outputs(hw, groups):
    from spatiotemporal_variable_separation_amd import ops
    shape = (4, 5) + hw
    C = shape[1]
    for x_dt, o_dt in ((F32, F32), (BF16, BF16), (F16, F16), (BF16, F32), (F16, F32)):     # same dtype, and mixed: 16-bit x, fp32 dy / out
        x, gamma, beta = _bn_inputs(shape, x_dt)
        dy = _rand(shape, 34, 1.0, o_dt)
        what = (hw, groups, x_dt, o_dt)

        def stats():
            rm, rv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
            return ops.bn_stats(x, rm, rv, 0.1, 1e-5, groups=groups) + (rm, rv)
        (mean, invstd, _, _), _, _ = _twice(stats, ('bn_stats',) + what)
        _twice(lambda: ops.bn_stats_ub(x, 1e-5, groups=groups), ('bn_stats_ub',) + what)
        for act in ('leaky_relu', 'sigmoid'):
            _twice(lambda: ops.bn_act_fwd(x, mean, invstd, gamma, beta, act, o_dt, groups=groups), ('bn_act_fwd', act) + what)
            for training in (True, False):
                _twice(lambda: ops.bn_act_bwd(dy, x, mean, invstd, gamma, beta, act, training, o_dt, groups=groups), ('bn_act_bwd', act, training) + what)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('shape', [(3, 40, 8, 8), (5, 33, 8, 24)])
def test_batchnorm_small_one_launch_forms_write_their_outputs(shape, dt):
    from spatiotemporal_variable_separation_amd import ops
    C = shape[1]
    x, gamma, beta = _bn_inputs(shape, dt)
    assert ops.bn_small_supported(x)

    def fwd(o_dt):
        rm, rv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
        return ops.bn_train_fwd_small(x, gamma, beta, 'leaky_relu', o_dt, rm, rv) + (rm, rv)
    for o_dt in (dt, F32):
        (y, mean, invstd, _, _), _, _ = _twice(lambda: fwd(o_dt), ('bn_train_fwd_small', shape, dt, o_dt))
        dy = _rand(shape, 35, 1.0, dt)
        _twice(lambda: ops.bn_act_bwd(dy, x, mean, invstd, gamma, beta, 'leaky_relu', True, o_dt), ('bn_act_bwd (small slabs)', shape, dt, o_dt))


@pytest.mark.parametrize('dt', [BF16, F16])
def test_batchnorm_register_resident_slab_forms_write_their_outputs(dt):
    from spatiotemporal_variable_separation_amd import ops
    shape, groups = (33, 5, 32, 32), 3
    C = shape[1]
    x, gamma, beta = _bn_inputs(shape, dt)
    assert ops.bn_slab_supported(x, groups)

    def fwd():
        rm, rv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
        return ops.bn_train_fwd_slab(x, gamma, beta, 'leaky_relu', dt, rm, rv, groups=groups) + (rm, rv)
    (y, mean, invstd, _, _), _, _ = _twice(fwd, ('bn_train_fwd_slab', dt))
    dy = _rand(shape, 36, 1.0, dt)
    _twice(lambda: ops.bn_act_bwd(dy, x, mean, invstd, gamma, beta, 'leaky_relu', True, dt, groups=groups), ('bn_act_bwd (resident slabs)', dt))


@pytest.mark.parametrize('dt', [BF16, F16])
def test_batchnorm_on_split_slabs_writes_its_outputs(dt):
    from spatiotemporal_variable_separation_amd import ops
    S, B, C, H, W = 2, 3, 40, 8, 8
    slabs, bias = _rand((S, B, C, H, W), 37), _rand((C,), 38)
    gamma, beta = 1 + _rand((C,), 39, 0.3), _rand((C,), 40, 0.2)
    skip = _rand((B, C, H, W), 41)

    def fwd(skip, want16, o_dt):
        rm, rv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
        return ops.bn_train_fwd_small_slabs(slabs, bias, dt, gamma, beta, 'leaky_relu', o_dt, rm, rv, skip=skip, want16=want16) + (rm, rv)
    _twice(lambda: fwd(None, False, dt), ('bn_train_fwd_small_slabs', dt))
    _twice(lambda: fwd(skip, False, F32), ('bn_train_fwd_small_slabs + skip', dt))
    (y, z, mean, invstd, *_), _, _ = _twice(lambda: fwd(skip, True, dt), ('bn_train_fwd_small_slabs + skip + want16', dt))
    # the backward's three gradient forms, stored and added to a pending gradient
    dy_a, dy_b = _rand((B, C, H, W), 42, 1.0, dt), _rand((B, C, H, W), 43)
    forms = {'slabs': dict(slabs=slabs), 'dy_a': dict(dy_a=dy_a), 'dy_a + dy_b': dict(dy_a=dy_a, dy_b=dy_b)}
    for name, kw in forms.items():
        for dx_dt in (dt, F32):
            _twice(lambda: ops.bn_act_bwd_small_ex(z, mean, invstd, gamma, beta, 'leaky_relu', dx_dt, **kw), ('bn_act_bwd_small_ex', name, dt, dx_dt))

            def acc():
                dg, db = torch.full((C,), 0.25, device='cuda'), torch.full((C,), -0.5, device='cuda')
                return ops.bn_act_bwd_small_ex(z, mean, invstd, gamma, beta, 'leaky_relu', dx_dt, acc=(dg, db), **kw) + (dg, db)
            _twice(acc, ('bn_act_bwd_small_ex + acc', name, dt, dx_dt))


# ------------------------------------------------------------------------------------------------------------------ pooling
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('shape', [(3, 5, 16, 16), (3, 5, 8, 12), (1, 3, 2, 2)])        # 16-byte forms / element forms
def test_pool_and_upsample_write_their_maps(shape, dt):
    from spatiotemporal_variable_separation_amd import ops
    B, C, H, W = shape
    x = _rand(shape, 50, 1.0, dt)
    dy_small, dy_big = _rand((B, C, H // 2, W // 2), 51, 1.0, dt), _rand((B, C, 2 * H, 2 * W), 52, 1.0, dt)
    _twice(lambda: ops.maxpool2_fwd(x), ('maxpool2_fwd', shape, dt))
    _twice(lambda: ops.maxpool2_bwd(x, dy_small), ('maxpool2_bwd', shape, dt))
    _twice(lambda: ops.upsample2_fwd(x), ('upsample2_fwd', shape, dt))
    _twice(lambda: ops.upsample2_bwd(dy_big, dt), ('upsample2_bwd', shape, dt))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('shape', [(1, 3, 5, 7), (2, 2, 1, 1)])
def test_maxpool3s2_writes_its_maps(shape, dt):
    from spatiotemporal_variable_separation_amd import ops
    B, C, H, W = shape
    x = _rand(shape, 53, 1.0, dt)
    dy = _rand((B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), 54, 1.0, dt)
    _twice(lambda: ops.maxpool3s2_fwd(x), ('maxpool3s2_fwd', shape, dt))
    _twice(lambda: ops.maxpool3s2_bwd(x, dy), ('maxpool3s2_bwd', shape, dt))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('shape', [(3, 5, 7, 7), (2, 1, 64, 64), (3, 5, 8, 8)])
def test_chan_sum_writes_c_sums(shape, dt):
    from spatiotemporal_variable_separation_amd import ops
    x = _rand(shape, 55, 1.0, dt)
    _twice(lambda: ops.chan_sum(x), ('chan_sum', shape, dt))


# ------------------------------------------------------------------------------------------------------------------ convolutions
# rows of GEOMS in tests/test_conv_gpu.py: (B, Cin, H, W, Cout, k, stride, pad, transposed)
CONV_GEOMS = [(1, 130, 8, 8, 70, 3, 1, 1, False), (2, 15, 64, 64, 16, 5, 2, 3, False), (3, 8, 17, 17, 12, 3, 2, 1, False), (3, 8, 32, 32, 1, 4, 2, 1, True),
              (4, 11, 1, 1, 16, 4, 1, 0, True), (2, 16, 8, 8, 8, 4, 2, 1, True), (16, 64, 32, 32, 64, 4, 2, 1, False)]


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('geom', CONV_GEOMS)
def test_conv_fwd_dgrad_wgrad_write_their_outputs(geom, dt):
    import test_conv_gpu as TC
    from spatiotemporal_variable_separation_amd import ops
    assert geom in TC.GEOMS
    B, Cin, H, W, Cout, k, s, p, tr = geom
    x = _rand((B, Cin, H, W), 60, 1.0, dt)
    wshape = (Cin, Cout, k, k) if tr else (Cout, Cin, k, k)
    w, bias = _rand(wshape, 61, 0.3, dt), _rand((Cout,), 62)
    for o_dt in (F32, dt):
        (y,), _, _ = _twice(lambda: ops.conv_fwd(x, w, bias, s, p, tr, o_dt), ('conv_fwd', geom, dt, o_dt))
        dy = _rand(tuple(y.shape), 63, 1.0, dt)
        _twice(lambda: ops.conv_dgrad(dy, w, x.shape, s, p, tr, o_dt), ('conv_dgrad', geom, dt, o_dt))
    _twice(lambda: ops.conv_wgrad(dy, x, wshape, s, p, tr), ('conv_wgrad', geom, dt))


# the direct kernels at the FIRST geometry of their parametrize lists in tests/test_conv_gpu.py
_SUMS = (1e-6, 1e-6)        # fp64 BatchNorm sums added with atomics in the epilogue: the bound of the tap kernels' own tests


@pytest.mark.parametrize('dt', [BF16, F16])
def test_tap_kernels_write_their_outputs(dt):
    from spatiotemporal_variable_separation_amd import ops
    B, Cin, H, Cout, groups = 32, 64, 4, 32, 2
    x, bias = _rand((B, Cin, H, H), 100, 1.0, dt), _rand((Cout,), 101)
    assert ops.convt_tap_supported(x, Cout, groups)
    wt = ops.convt_tap_pack_weight(_rand((Cin, Cout, 4, 4), 102, 0.3), dt)
    _twice(lambda: ops.convt_tap_fwd(x, wt, bias, Cout, groups=groups), ('convt_tap_fwd', dt), loose={1: _SUMS})
    Cout = 40
    bias = _rand((Cout,), 103)
    assert ops.conv_k3_tap_supported(x, Cout, groups, force=True)
    w3 = ops.conv_k3_tap_pack_weight(_rand((Cout, Cin, 3, 3), 104, 0.3), dt, False)
    _twice(lambda: ops.conv_k3_tap_fwd(x, w3, bias, Cout, dt, groups=groups, want_sums=True), ('conv_k3_tap_fwd', dt), loose={1: _SUMS})
    _twice(lambda: ops.conv_k3_tap_fwd(x, w3, bias, Cout, F32), ('conv_k3_tap_fwd fp32', dt))


@pytest.mark.parametrize('dt', [BF16, F16])
def test_conv3_kernels_write_their_outputs(dt, monkeypatch):
    from spatiotemporal_variable_separation_amd import ops
    B, Cin, Cout = 8, 512, 512                                          # vs_conv3_img16: split slabs
    x = _rand((B, Cin, 16, 16), 105, 1.0, dt)
    assert ops.conv3_img16_supported(x, Cout)
    wp = ops.conv3_img16_pack_weight(_rand((Cout, Cin, 3, 3), 106, 0.3), dt, False)
    _twice(lambda: ops.conv3_img16(x, wp, Cout), ('conv3_img16', dt))
    B, Cin, H, W, Cout = 2, 64, 64, 64, 64                              # vs_conv3_band, vs_conv3_wgrad_band
    x, bias = _rand((B, Cin, H, W), 107, 1.0, dt), _rand((Cout,), 108)
    assert ops.conv3_band_supported(x, Cout)
    wp = ops.conv3_img16_pack_weight(_rand((Cout, Cin, 3, 3), 109, 0.3), dt, False)
    for o_dt in (F32, dt):
        _twice(lambda: ops.conv3_band(x, wp, bias, Cout, o_dt), ('conv3_band', dt, o_dt))
    monkeypatch.setenv('VS_CONV_WGRAD_BAND', '1')
    dz = _rand((B, Cout, H, W), 110, 1.0, dt)
    assert ops.conv3_wgrad_band_supported(x, Cout)
    _twice(lambda: ops.conv_wgrad(dz, x, (Cout, Cin, 3, 3), 1, 1, False), ('conv3_wgrad_band', dt))


@pytest.mark.parametrize('dt', [BF16, F16])
def test_conv_k4s2_on_parity_planes_writes_its_outputs(dt):
    from spatiotemporal_variable_separation_amd import ops
    B, C, H, W, M = 6, 64, 32, 32, 128
    x, bias = _rand((B, C, H, W), 111, 1.0, dt), _rand((M,), 112)
    assert ops.conv_k4s2_supported(x, M)
    (planes,), _, _ = _twice(lambda: ops.space_to_depth2(x), ('space_to_depth2', dt))
    wp = ops.conv_k4s2_pack_weight(_rand((M, C, 4, 4), 113, 0.3), dt)
    for o_dt in (F32, dt):
        _twice(lambda: ops.conv_k4s2_gather(planes, wp, bias, M, o_dt), ('conv_k4s2_gather', dt, o_dt))
    _twice(lambda: ops.conv_k4s2_gather(planes, wp, None, M, F32, role='dgrad'), ('conv_k4s2_gather dgrad', dt))
    dz = _rand((B, M, H // 2, W // 2), 114, 1.0, dt)
    _twice(lambda: ops.conv_k4s2_wgrad(dz, planes, (M, C, 4, 4)), ('conv_k4s2_wgrad', dt))


@pytest.mark.parametrize('dt', [BF16, F16])
@pytest.mark.parametrize('gi,kernels', [(0, {'fwd': 'expand', 'dgrad': None, 'wgrad': 'wgrad_big_dy'}),
                                        (4, {'fwd': 'reduce', 'dgrad': 'expand', 'wgrad': 'wgrad_big_x'})])
def test_conv_thin_kernels_write_their_outputs(gi, kernels, dt):
    """THIN_GEOMS[0] (Conv2d from 5 thin channels): the forward is the expand kernel and the weight gradient the thin one; its input gradient
    has NO thin plan (64 output channels) and runs another family.  THIN_GEOMS[4] (ConvTranspose2d onto 1 thin channel) adds the reduce
    kernel (forward), expand as an input gradient and the other weight-gradient form.  Which kernel serves what is asserted from
    ops._thin_plan, as tests/test_conv_gpu.py does."""
    import test_conv_gpu as TC
    from spatiotemporal_variable_separation_amd import ops
    from spatiotemporal_variable_separation_amd._lib import code_of
    B, Cin, H, W, Cout, k, s, p, tr = TC.THIN_GEOMS[gi]
    x = _rand((B, Cin, H, W), 115, 1.0, dt)
    wshape = (Cin, Cout, k, k) if tr else (Cout, Cin, k, k)
    w, bias = _rand(wshape, 116, 0.3, dt), _rand((Cout,), 117)
    OH, OW = ((H - 1) * s - 2 * p + k, (W - 1) * s - 2 * p + k) if tr else ((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1)
    dy = _rand((B, Cout, OH, OW), 118, 1.0, dt)
    plans = {op: ops._thin_plan(op, code_of(dt), B, Cin, H, W, Cout, OH, OW, k, s, p, tr, wgrad_max_m=8) for op in ('fwd', 'dgrad', 'wgrad')}
    assert {op: (pl[0] if pl is not None else None) for op, pl in plans.items()} == kernels, plans
    for o_dt in (F32, dt):
        (y,), _, _ = _twice(lambda: ops.conv_fwd(x, w, bias, s, p, tr, o_dt), ('conv_thin fwd', gi, dt, o_dt))
        assert tuple(y.shape) == (B, Cout, OH, OW)
        _twice(lambda: ops.conv_dgrad(dy, w, x.shape, s, p, tr, o_dt), ('conv_thin dgrad', gi, dt, o_dt))
    big, small = (dy, x) if plans['wgrad'][0] == 'wgrad_big_dy' else (x, dy)
    _twice(lambda: ops.conv_thin_wgrad(big, small, wshape, k, s, *plans['wgrad'][5:]), ('conv_thin_wgrad', gi, dt))


# ------------------------------------------------------------------------------------------- pointers off 16-byte alignment
# entry point -> (class, outcome, why[, what the refusal says]).  Class 1: the host tests the pointers and selects an element-wise form (or the planner falls
# through); class 2: the host refuses and says so.  There is no class 3 (wide accesses that nothing tests) left: vs_cast, vs_act_fwd,
# vs_act_bwd (map4), vs_frames_sse_fwd / _bwd and vs_bn_act_bwd's 16-byte-chunk form were of that class and test their pointers now.  A refusal is matched on the return code and the
# reason the host gives ('<entry> failed (<code>): <entry>: <reason>'), not on the entry point's name alone.
ERR_ARG, ERR_UNSUPPORTED = -1, -4          # VS_ERR_ARG, VS_ERR_UNSUPPORTED (include/varsep_hip.h)
MISALIGNED = {
    'vs_bn_stats': (1, 'ok', 'vec needs x % 16 == 0, else element by element'),
    'vs_bn_stats_ub': (1, 'ok', 'as vs_bn_stats'),
    'vs_bn_act_fwd': (1, 'ok', 'vec 1 / 2 need x and y % 16 == 0'),
    'vs_bn_act_fwd_running': (1, 'ok', 'as vs_bn_act_fwd'),
    'vs_bn_act_bwd': (1, 'ok', 'every vector form needs x, dy, dx % 16 == 0 (the 16-byte-chunk form did not test it before)'),
    'vs_maxpool2_fwd': (1, 'ok', 'v8_ok tests every pointer'),
    'vs_maxpool2_bwd': (1, 'ok', 'v8_ok'),
    'vs_upsample2_fwd': (1, 'ok', 'v8_ok'),
    'vs_upsample2_bwd': (1, 'ok', 'v8_ok'),
    'vs_maxpool3s2_fwd': (1, 'ok', 'element accesses only'),
    'vs_maxpool3s2_bwd': (1, 'ok', 'element accesses only'),
    'vs_colsum': (1, 'ok', 'element accesses only'),
    'vs_colsum_multi': (1, 'ok', 'vec needs X % 16 == 0 and ldx % 8 == 0'),
    'vs_copy2d': (1, 'ok', 'element accesses only'),
    'vs_copy2d_pair': (1, 'ok', 'the four-element form needs src and dst aligned to four elements'),
    'vs_transpose_cast': (1, 'ok', 'element accesses only'),
    'vs_cast': (1, 'ok', 'map4 takes its element loop unless src and dst are aligned to four elements (was class 3)'),
    'vs_act_fwd': (1, 'ok', 'as vs_cast (was class 3)'),
    'vs_act_bwd': (1, 'ok', 'as vs_cast; y is read element by element (was class 3)'),
    'vs_frames_sse_bwd': (1, 'ok', 'four-element form needs D % 4 == 0 and frames, full, dframes % 16 == 0 (was class 3)'),
    'vs_frames_sse_fwd': (1, 'ok', 'as vs_frames_sse_bwd: rows_vec_ok(frames), rows_vec_ok(full) (was class 3)'),
    'vs_mix_codes_fwd': (1, 'ok', 'element accesses only'),
    'vs_mix_codes_bwd': (1, 'ok', 'element accesses only'),
    'vs_gemm': (1, 'ok', 'tests/test_gemm_strided_gpu.py: the DMA families fall through to the register tile, whose loads and epilogue test the pointers'),
    'vs_gemm_batched': (1, 'ok', 'tests/test_gemm_strided_gpu.py: as vs_gemm, batch strides included'),
    'vs_chan_sum_ws': (2, 'refused', 'a 16-bit x with HW % 8 == 0 must be 16-byte aligned; fp32, or HW % 8 != 0: element accesses, ok', (ERR_ARG, 'vs_chan_sum_ws: .*a 16-bit operand must be 16-byte aligned')),
    'vs_cat_bcast_fwd': (2, 'refused', '16-byte aligned tensors, planes of a multiple of 8 elements', (ERR_ARG, 'vs_cat_bcast_fwd: .*16-byte aligned tensors')),
    'vs_cat_bcast_bwd': (2, 'refused', 'as vs_cat_bcast_fwd', (ERR_ARG, 'vs_cat_bcast_bwd: .*16-byte aligned tensors')),
    'vs_code_losses_fwd': (2, 'refused', 'pairs 16-byte aligned, counts multiples of 8', (ERR_ARG, 'vs_code_losses_fwd: .*16-byte aligned')),
    'vs_code_losses_bwd': (2, 'refused', 'as vs_code_losses_fwd', (ERR_ARG, 'vs_code_losses_bwd: .*16-byte aligned')),
    'vs_bn_stats_from_parts_fold': (2, 'refused', 'the table must be 8-byte aligned', (ERR_ARG, 'vs_bn_stats_from_parts_fold: .*the table must be 8-byte aligned')),
    'vs_slab_sum': (2, 'refused', 'operands must be 16-byte aligned', (ERR_ARG, 'vs_slab_sum: .*operands must be 16-byte aligned')),
    'vs_bn_train_fwd_small': (2, 'refused', 'VS_ERR_UNSUPPORTED: tensor not served (the caller takes vs_bn_stats + vs_bn_act_fwd)', (ERR_UNSUPPORTED, 'vs_bn_train_fwd_small: .*tensor not served')),
    'vs_bn_train_fwd_slab': (2, 'refused', 'VS_ERR_UNSUPPORTED: tensor not served', (ERR_UNSUPPORTED, 'vs_bn_train_fwd_slab: .*tensor not served')),
    'vs_bn_train_fwd_small_slabs': (2, 'refused', 'VS_ERR_UNSUPPORTED: tensor not served', (ERR_UNSUPPORTED, 'vs_bn_train_fwd_small_slabs: .*tensor not served')),
    'vs_bn_act_bwd_small_ex': (2, 'refused', 'VS_ERR_UNSUPPORTED: tensor not served', (ERR_UNSUPPORTED, 'vs_bn_act_bwd_small_ex: .*tensor not served')),
}


def _off(t):
    """`t` one element off its 512-byte-aligned buffer: contiguous, same values, data_ptr % 16 == element size."""
    from guard_util import embed
    v, _ = embed(t, offset=1)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size() and torch.equal(v, t)
    return v


def _close(dt, act_bound=2e-6):
    """Relative L2 bound between the aligned and the misaligned call of one operation: the existing fp32 bound of that call, or one rounding of
    a 16-bit result (6e-3 bf16 / 8e-4 fp16, tests/test_gemm_gpu.py)."""
    return {BF16: 6e-3, F16: 8e-4}.get(dt, act_bound)


def _mis(entry, aligned_fn, off_fn, bound=None, exact=False):
    """One row of MISALIGNED, run: aligned inputs and outputs vs inputs one element off and outputs one element off, guards checked."""
    from guard_util import guarded_ops
    from spatiotemporal_variable_separation_amd import _lib
    cls, outcome = MISALIGNED[entry][:2]
    with pytest.MonkeyPatch.context() as mp:
        allocs = guarded_ops(mp, misalign=1)
        if outcome == 'refused':
            code, says = MISALIGNED[entry][3]
            with pytest.raises(_lib.VarsepHipError, match=r'failed \(%d\): %s' % (code, says)):
                off_fn()
            torch.cuda.synchronize()
            allocs.check()
            for g in allocs.guards:                                      # nothing launched: every output is still all 0xFF
                assert bool((g.buf == 0xFF).all()), (entry, 'refused, but allocation #%d was written' % g.ordinal)
            return None
        got = _flat(off_fn())
        torch.cuda.synchronize()
    allocs.check()
    want = _flat(aligned_fn())
    assert len(got) == len(want) and allocs.guards and all((a.buf.data_ptr() + a.start) % 16 != 0 for a in allocs.guards), entry
    for i, (g, w) in enumerate(zip(got, want)):
        assert not bool(torch.isnan(g.double()).any()), (entry, 'output %d holds NaN' % i)
        if exact:
            assert torch.equal(g, w), (entry, i, (g.double() - w.double()).abs().max().item())
        else:
            err = ((g.double() - w.double()).norm() / (w.double().norm() + 1e-30)).item()
            assert err < (bound if bound is not None else _close(g.dtype)), (entry, i, err)
    return got


@pytest.mark.parametrize('dt', DTYPES)
def test_misaligned_batchnorm(dt):
    """HW = 64 (the shape at which alignment alone decides the form), x / dy one element off, every output one element off."""
    from spatiotemporal_variable_separation_amd import ops
    shape, C = (4, 5, 8, 8), 5
    x, gamma, beta = _bn_inputs(shape, dt)
    dy = _rand(shape, 70, 1.0, dt)
    xo, dyo = _off(x), _off(dy)
    for groups in (1, 2):
        mean, invstd = ops.bn_stats(x, groups=groups)
        _mis('vs_bn_stats', lambda: ops.bn_stats(x, groups=groups), lambda: ops.bn_stats(xo, groups=groups), bound=2e-6)
        _mis('vs_bn_stats_ub', lambda: ops.bn_stats_ub(x, groups=groups), lambda: ops.bn_stats_ub(xo, groups=groups), bound=2e-6)
        for o_dt in (dt, F32):
            _mis('vs_bn_act_fwd', lambda: ops.bn_act_fwd(x, mean, invstd, gamma, beta, 'leaky_relu', o_dt, groups=groups),
                 lambda: ops.bn_act_fwd(xo, mean, invstd, gamma, beta, 'leaky_relu', o_dt, groups=groups))

            def running(xx):
                ub = ops.bn_stats_ub(x, groups=groups)[2]
                rm, rv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
                return ops.bn_act_fwd(xx, mean, invstd, gamma, beta, 'leaky_relu', o_dt, groups=groups, running=(ub, rm, rv, 0.1)), rm, rv
            _mis('vs_bn_act_fwd_running', lambda: running(x), lambda: running(xo))
            for training in (True, False):
                # (dx, dgamma, dbeta): the bound of test_batchnorm_act_fwd_bwd for the backward, 2e-5
                _mis('vs_bn_act_bwd', lambda: ops.bn_act_bwd(dy, x, mean, invstd, gamma, beta, 'leaky_relu', training, o_dt, groups=groups),
                     lambda: ops.bn_act_bwd(dyo, xo, mean, invstd, gamma, beta, 'leaky_relu', training, o_dt, groups=groups), bound=_close(o_dt, 2e-5))
        if dt != F32:                                                    # mixed: 16-bit x, fp32 dy and dx (aligned: the unit-per-plane form, vec 2)
            dy32 = _rand(shape, 69)
            dy32o = _off(dy32)
            for training in (True, False):
                _mis('vs_bn_act_bwd', lambda: ops.bn_act_bwd(dy32, x, mean, invstd, gamma, beta, 'leaky_relu', training, F32, groups=groups),
                     lambda: ops.bn_act_bwd(dy32o, xo, mean, invstd, gamma, beta, 'leaky_relu', training, F32, groups=groups), bound=2e-5)


@pytest.mark.parametrize('dt', DTYPES)
def test_misaligned_batchnorm_one_launch_forms_are_refused(dt):
    from spatiotemporal_variable_separation_amd import ops
    shape, C = (3, 40, 8, 8), 40
    x, gamma, beta = _bn_inputs(shape, dt)
    xo = _off(x)
    _mis('vs_bn_train_fwd_small', None, lambda: ops.bn_train_fwd_small(xo, gamma, beta, 'leaky_relu', dt))
    if dt == F32:
        return
    slabs, bias = _rand((2,) + shape, 71), _rand((C,), 72)
    _mis('vs_bn_train_fwd_small_slabs', None, lambda: ops.bn_train_fwd_small_slabs(_off(slabs), bias, dt, gamma, beta, 'leaky_relu', dt))
    _mis('vs_slab_sum', None, lambda: ops.slab_sum(_off(slabs), bias, dt))
    mean, invstd = ops.bn_stats(x)
    _mis('vs_bn_act_bwd_small_ex', None, lambda: ops.bn_act_bwd_small_ex(xo, mean, invstd, gamma, beta, 'leaky_relu', dt, dy_a=xo))
    big = _rand((33, 5, 32, 32), 73, 1.0, dt)
    _mis('vs_bn_train_fwd_slab', None, lambda: ops.bn_train_fwd_slab(_off(big), gamma[:5].contiguous(), beta[:5].contiguous(), 'leaky_relu', dt, groups=3))
    parts = _rand((6, C, 2), 74)
    _mis('vs_bn_stats_from_parts_fold', None, lambda: ops.bn_stats_from_parts_fold(_off(parts), 2, 64))


@pytest.mark.parametrize('dt', DTYPES)
def test_misaligned_pooling(dt):
    from spatiotemporal_variable_separation_amd import ops
    shape = (3, 5, 16, 16)
    x = _rand(shape, 75, 1.0, dt)
    dy_small, dy_big = _rand((3, 5, 8, 8), 76, 1.0, dt), _rand((3, 5, 32, 32), 77, 1.0, dt)
    xo, so, bo = _off(x), _off(dy_small), _off(dy_big)
    _mis('vs_maxpool2_fwd', lambda: ops.maxpool2_fwd(x), lambda: ops.maxpool2_fwd(xo), exact=True)
    _mis('vs_maxpool2_bwd', lambda: ops.maxpool2_bwd(x, dy_small), lambda: ops.maxpool2_bwd(xo, so), exact=True)
    _mis('vs_upsample2_fwd', lambda: ops.upsample2_fwd(x), lambda: ops.upsample2_fwd(xo), exact=True)
    _mis('vs_upsample2_bwd', lambda: ops.upsample2_bwd(dy_big, dt), lambda: ops.upsample2_bwd(bo, dt))      # (a sum of four: one rounding)
    _mis('vs_maxpool3s2_fwd', lambda: ops.maxpool3s2_fwd(x), lambda: ops.maxpool3s2_fwd(xo), exact=True)
    _mis('vs_maxpool3s2_bwd', lambda: ops.maxpool3s2_bwd(x, dy_small), lambda: ops.maxpool3s2_bwd(xo, so))


@pytest.mark.parametrize('dt', DTYPES)
def test_misaligned_element_wise(dt):
    from guard_util import embed, window
    from spatiotemporal_variable_separation_amd import ops
    n = 1029
    x, dy = _rand((n,), 78, 3.0, dt), _rand((n,), 79, 3.0, dt)
    xo, dyo = _off(x), _off(dy)
    for o_dt in DTYPES:
        _mis('vs_cast', lambda: ops.cast(x, o_dt), lambda: ops.cast(xo, o_dt), exact=True)
        _mis('vs_act_fwd', lambda: ops.act_fwd(x, 'relu', out_dtype=o_dt), lambda: ops.act_fwd(xo, 'relu', out_dtype=o_dt), exact=True)
        _mis('vs_act_bwd', lambda: ops.act_bwd(dy, x, 'relu', out_dtype=o_dt), lambda: ops.act_bwd(dyo, xo, 'relu', out_dtype=o_dt), exact=True)
        # sigmoid: the bound of test_colsum_cast_act (1e-6), one rounding for a 16-bit result
        _mis('vs_act_fwd', lambda: ops.act_fwd(x, 'sigmoid', out_dtype=o_dt), lambda: ops.act_fwd(xo, 'sigmoid', out_dtype=o_dt), bound=_close(o_dt, 1e-6))
    # aligned input, misaligned output only -- and the other way round
    from guard_util import guarded_ops
    with pytest.MonkeyPatch.context() as mp:
        allocs = guarded_ops(mp, misalign=1)
        got = ops.cast(x, BF16)
    allocs.check()
    assert got.data_ptr() % 16 == 2 and torch.equal(got, x.to(BF16))
    assert torch.equal(ops.cast(xo, BF16), x.to(BF16))
    m = _rand((33, 65), 80, 1.0, dt)
    _mis('vs_transpose_cast', lambda: ops.transpose_cast(m, F32), lambda: ops.transpose_cast(_off(m), F32), exact=True)
    _mis('vs_colsum', lambda: ops.colsum(m, 33, 65), lambda: ops.colsum(_off(m), 33, 65), bound=2e-6)
    j = _rand((300, 264), 81, 1.0, dt)
    _mis('vs_colsum_multi', lambda: ops.colsum_multi([j, m]), lambda: ops.colsum_multi([_off(j), _off(m)]), bound=2e-6)
    # copy2d / copy2d_pair write into the caller's window
    src = _rand((8, 24), 82, 1.0, dt)
    so = _off(src)
    off = torch.tensor([1], dtype=torch.int32, device='cuda')
    for o_dt in DTYPES:
        out, g = window((7, 12), o_dt, ld=16, offset=1, device='cuda', rows_before=1)
        ops.copy2d(so, 7, 12, 24, out, 16)
        g.check()
        assert torch.equal(out, src[:7, :12].to(o_dt))
        out, g = window((14, 12), o_dt, ld=16, offset=1, device='cuda', rows_before=1)
        ops.copy2d_pair(so, 7, 12, 24, out, 16, off, 4, 0, 8)
        g.check()
        assert torch.equal(out, torch.cat([src[:7, 4:16], src[:7, 8:20]]).to(o_dt))
    assert MISALIGNED['vs_copy2d'][1] == MISALIGNED['vs_copy2d_pair'][1] == 'ok'
    if dt == F32:
        B, G, T, D = 3, 2, 4, 64
        frames, full = _rand((B, G, D), 83), _rand((B, T, D), 84)
        idx = torch.tensor([1, 3], dtype=torch.int32, device='cuda')
        coef = torch.tensor([0.5, -0.25], device='cuda')
        _mis('vs_frames_sse_bwd', lambda: ops.frames_sse_bwd(frames, full, idx, coef), lambda: ops.frames_sse_bwd(_off(frames), _off(full), idx, coef), exact=True)
        # the forward's two sums: float atomics over the workgroups (last-bit nondeterminism) -- rtol 1e-5 against fp64, as below
        _mis('vs_frames_sse_fwd', lambda: ops.frames_sse_fwd(frames, full, idx), lambda: ops.frames_sse_fwd(_off(frames), _off(full), idx), bound=1e-5)
        ref = torch.stack([((frames[:, 0] - full[:, 1]).double() ** 2).sum(), ((frames[:, 1] - full[:, 3]).double() ** 2).sum()])
        assert torch.allclose(ops.frames_sse_fwd(_off(frames), full, idx).double(), ref, rtol=1e-5)
        B, n, Cs = 5, 3, 7
        s_, t_rand, t_codes, dz = _rand((B, Cs), 14), _rand((B, Cs), 15), _rand((B, n, Cs), 16), _rand((B, n + 1, Cs), 17)
        _mis('vs_mix_codes_fwd', lambda: ops.mix_codes_fwd(s_, t_rand, t_codes, 'mul', lowp=BF16),
             lambda: ops.mix_codes_fwd(_off(s_), _off(t_rand), _off(t_codes), 'mul', lowp=BF16), exact=True)
        _mis('vs_mix_codes_bwd', lambda: ops.mix_codes_bwd(dz, s_, t_rand, t_codes, 'mul'),
             lambda: ops.mix_codes_bwd(_off(dz), _off(s_), _off(t_rand), _off(t_codes), 'mul'), exact=True)
        for d in (63, 5):                                                # rows that no 16-byte access fits, aligned base
            f2, u2 = _rand((B, G, d), 85), _rand((B, T, d), 86)
            want = torch.stack([coef[0] * (f2[:, 0] - u2[:, 1]), coef[1] * (f2[:, 1] - u2[:, 3])], dim=1)
            (got,), _, _ = _twice(lambda: ops.frames_sse_bwd(f2, u2, idx, coef), ('frames_sse_bwd', d))
            assert torch.equal(got, want)
            sums = ops.frames_sse_fwd(f2, u2, idx)
            ref = torch.stack([((f2[:, 0] - u2[:, 1]).double() ** 2).sum(), ((f2[:, 1] - u2[:, 3]).double() ** 2).sum()])
            assert torch.allclose(sums.double(), ref, rtol=1e-5), (d, sums, ref)


@pytest.mark.parametrize('dt', DTYPES)
def test_misaligned_chan_sum_cat_bcast_and_code_losses(dt):
    from spatiotemporal_variable_separation_amd import _lib, ops
    x8, x7 = _rand((3, 5, 8, 8), 87, 1.0, dt), _rand((3, 5, 7, 7), 88, 1.0, dt)
    if dt != F32:
        _mis('vs_chan_sum_ws', None, lambda: ops.chan_sum(_off(x8)))
    from guard_util import guarded_ops
    for x in ((x8, x7) if dt == F32 else (x7,)):                         # HW % 8 != 0 (and fp32): element accesses -- accepted, and must be right
        with pytest.MonkeyPatch.context() as mp:
            allocs = guarded_ops(mp, misalign=1)
            got = ops.chan_sum(_off(x))
        allocs.check()
        assert torch.equal(got, ops.chan_sum(x)), 'fixed summation order: the misaligned call gives the same bits'
        ref = x.double().sum((0, 2, 3))
        assert ((got.double() - ref).norm() / ref.norm()).item() < 2e-6
    B, n, Ca, Cb = 2, 3, 3, 2
    a, xx, dout = _rand((B, Ca, 8, 8), 89, 1.0, dt), _rand((n * B, Cb, 8, 8), 90, 1.0, dt), _rand((n * B, Ca + Cb, 8, 8), 91, 1.0, dt)
    assert not ops.cat_bcast_supported(_off(a), xx, n)
    _mis('vs_cat_bcast_fwd', None, lambda: ops.cat_bcast_fwd(_off(a), xx, n, dt))
    _mis('vs_cat_bcast_bwd', None, lambda: ops.cat_bcast_bwd(_off(dout), B, n, Ca, dt, dt))
    p, q, t0 = _rand((4, 16), 92, 1.0, dt), _rand((4, 16), 93, 1.0, dt), _rand((4, 8), 94)
    sse = torch.ones(2, device='cuda')
    po = _off(p)
    assert ops.code_losses_supported([(p, q)], t0) and not ops.code_losses_supported([(po, q)], t0)
    _mis('vs_code_losses_fwd', None, lambda: ops.code_losses_fwd([(po, q)], t0, sse, sse, 1.0, 1.0, (1, 1, 1, 1), 0.25))
    g = torch.ones(1, device='cuda')
    _mis('vs_code_losses_bwd', None, lambda: ops.code_losses_bwd([(po, q)], [(True, True)], t0, g, 1.0, 1.0, (1, 1, 1, 1), 0.25))


def test_a_17x17_batch_slice_goes_through_batchnorm_and_cast():
    """x[1:] of a (3, 5, 17, 17) bf16 tensor: contiguous and 2890 bytes (% 16 == 10) past its allocation -- the chairs ResNet's case."""
    from spatiotemporal_variable_separation_amd import ops
    whole = _rand((3, 5, 17, 17), 95, 2.0, BF16)
    x = whole[1:]
    assert x.is_contiguous() and x.data_ptr() % 16 == 10
    dense = x.clone()
    assert dense.data_ptr() % 16 == 0
    gamma, beta = 1 + _rand((5,), 96, 0.3), _rand((5,), 97, 0.2)
    dy_whole = _rand((3, 5, 17, 17), 98, 1.0, BF16)
    dy, dy_dense = dy_whole[1:], dy_whole[1:].clone()

    def rel(a, b):
        return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()
    mean, invstd = ops.bn_stats(x)
    mean_d, invstd_d = ops.bn_stats(dense)
    assert rel(mean, mean_d) < 2e-6 and rel(invstd, invstd_d) < 2e-6
    for o_dt in (BF16, F32):
        y, y_d = (ops.bn_act_fwd(t, mean_d, invstd_d, gamma, beta, 'leaky_relu', o_dt) for t in (x, dense))
        assert rel(y, y_d) < _close(o_dt)
        got = ops.bn_act_bwd(dy, x, mean_d, invstd_d, gamma, beta, 'leaky_relu', True, o_dt)
        want = ops.bn_act_bwd(dy_dense, dense, mean_d, invstd_d, gamma, beta, 'leaky_relu', True, o_dt)
        for g, w in zip(got, want):
            assert rel(g, w) < _close(g.dtype, 2e-5)
    for o_dt in DTYPES:
        assert torch.equal(ops.cast(x, o_dt), dense.to(o_dt))
    # and with every output off alignment as well
    from guard_util import guarded_ops
    with pytest.MonkeyPatch.context() as mp:
        allocs = guarded_ops(mp, misalign=1)
        y = ops.bn_act_fwd(x, mean_d, invstd_d, gamma, beta, 'leaky_relu', BF16)
        dx, dg, db = ops.bn_act_bwd(dy, x, mean_d, invstd_d, gamma, beta, 'leaky_relu', True, BF16)
        c = ops.cast(x, F32)
    allocs.check()
    assert rel(y, ops.bn_act_fwd(dense, mean_d, invstd_d, gamma, beta, 'leaky_relu', BF16)) < _close(BF16)
    for g, w in zip((dx, dg, db), ops.bn_act_bwd(dy_dense, dense, mean_d, invstd_d, gamma, beta, 'leaky_relu', True, BF16)):
        assert rel(g, w) < _close(g.dtype, 2e-5)
    assert torch.equal(c, dense.float())


def test_a_byte_written_behind_an_output_on_the_device_is_reported():
    """The positive control of this file: one element stored right behind a guarded output fails the check and names the allocation."""
    from guard_util import guarded_ops
    from spatiotemporal_variable_separation_amd import ops
    x = _rand((1029,), 99)
    with pytest.MonkeyPatch.context() as mp:
        allocs = guarded_ops(mp)
        y = ops.cast(x, BF16)
    allocs.check()
    torch.as_strided(y, (1,), (1,), y.storage_offset() + 1029).fill_(1.0)                   # the element after the last one
    with pytest.raises(AssertionError, match=r'allocation #0 \(shape \(1029,\), torch.bfloat16\): 2 guard byte\(s\) overwritten, the first after the window'):
        allocs.check()


def test_every_row_of_the_table_has_a_class_and_an_outcome():
    assert all(row[0] in (1, 2) and row[1] in ('ok', 'refused') and row[2] for row in MISALIGNED.values())
    assert all((row[0] == 2) == (row[1] == 'refused') == (len(row) == 4) for row in MISALIGNED.values())

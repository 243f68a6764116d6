"""Which kernels `functional.ConvBlock` launches, in which order and with which arguments, and what it keeps for backward: every case of
tests/make_golden_conv_block_routes.py replayed on the CPU and compared EXACTLY with tests/golden/conv_block_routes.json (the launch names
of every case as text, everything else through a digest of the case's full record; a case that moves is printed in full).

The launching `ops` functions are the recording stand-ins of tests/ops_standins.py; the `*_supported`, `*_enabled` and `band_bn_mode` functions
are the real host-only calls into the built library, so a row that moves is a layer that changed route (or launch order, or an argument).  The
fixture was written by the if / elif ladder ConvBlock.forward was before its split into route choice, conv stage and BatchNorm tail.

Reached by the fixture (asserted below): the forward routes k4_planes, k4_gather (BatchNorm only), img16, band, tap and cols behind a training-mode
BatchNorm and without one, both epilogue-statistics forms (fp64 sums, partial-sum table) on the band and on the k4 planes, the slab form of img16, the one-launch small
BatchNorm, the slab-in-registers form, both statistics passes, the eval-mode tail, the input-gradient routes dz_planes, tap, img16, band and
conv_dgrad, both k4 weight-gradient forms (planes kept by forward, planes of dz).

NOT reached, because the real `*_supported` functions never select them on the CPU either (a scan over batch, channels and map sizes found no
shape): k3tap as forward and as input-gradient route (`conv3_img16_supported` or `conv3_band_supported` holds wherever `conv_k3_tap_supported`
does: the band serves every 4x4 / 8x8 / 16x16 map with Cin >= 384 and Cout >= 256).  The GPU tests of the tap
kernel itself (tests/test_conv_gpu.py) are what covers that code.
"""
import json

import pytest

import make_golden_conv_block_routes as G


@pytest.fixture(scope='module')
def golden():
    """{key: full record} of every case as the code stands, replayed once for the module.  test_every_case_replays_the_fixture_exactly says that
    this IS the committed fixture; the named decisions below read it."""
    return G.replay()


def test_every_case_replays_the_fixture_exactly(golden):
    with open(G.PATH) as f:
        moved = G.moved(golden, json.load(f))
    for key, what, now, was in moved[:5]:
        print('%s: %s\n  now    %s\n  stored %s\n  full record now: %s' % (key, what, now, was, golden[key]))
    assert not moved, '%d of %d cases moved, e.g. %s' % (len(moved), len(golden), [m[:2] for m in moved[:5]])


def test_the_fixture_reaches_every_route_and_tail(golden):
    seen = G.coverage(golden)
    assert not [label for label in G.REQUIRED if label not in seen]
    assert 'tail:bn_stats' in seen and 'tail:bn_stats_ub' in seen and 'tail:bn_train_fwd_slab' in seen


def test_the_product_of_factors_is_there(golden):
    keys = [k.split('|') for k in golden]
    assert {k[0] for k in keys} == {'bf16', 'fp16', 'fp32'}
    assert {k[1] for k in keys if k[0] == 'bf16'} == set(G.LAYERS)
    for position, values in ((2, {'bn=train', 'bn=train_untracked', 'bn=eval', 'bn=none'}), (4, {'o32=0', 'o32=1'}), (5, {'xlowp=0', 'xlowp=1'}),
                             (6, {'xg=0', 'xg=1'}), (7, {'wg=0', 'wg=1'}), (8, {'sums=', 'sums=1', 'sums=parts'}), (9, {'small=', 'small=1'})):
        assert {k[position] for k in keys} == values
    assert {k[3] for k in keys} == {'g=1', 'g=2'}


# ------------------------------------------------------------------------------------------------------------------ named decisions
def record(golden, layer, precision='bf16', bn='train', g=1, o32=0, xlowp=0, xg=1, wg=1, sums='', small=''):
    key = '%s|%s|bn=%s|g=%d|o32=%d|xlowp=%d|xg=%d|wg=%d|sums=%s|small=%s' % (precision, layer, bn, g, o32, xlowp, xg, wg, sums, small)
    return golden[key]


def fwd(r):
    return [n for n in G.names(r['forward']) if n != 'cast' and not n.endswith('pack_weight')]


def bwd(r):
    return [n for n in G.names(r['backward']) if n != 'cast' and not n.endswith('pack_weight')]


def test_taxibj_32x32_3x3_layer_in_bf16_takes_band_with_a_statistics_pass(golden):
    # (two stacked calls, as the TaxiBJ step issues them)
    r = record(golden, 'taxibj_vgg_32', g=2)
    assert fwd(r) == ['conv3_band', 'bn_stats_ub', 'bn_act_fwd']
    assert r['saved'][1] == ['bf16', [12, 64, 32, 32]] and r['result'] == ['bf16', [12, 64, 32, 32]]
    assert bwd(r) == ['bn_act_bwd', 'conv_wgrad', 'conv3_band']
    assert fwd(record(golden, 'taxibj_vgg_32', g=2, bn='eval')) == ['conv3_band', 'bn_act_fwd']
    # one call of twelve maps: a (call, channel) slab fits one workgroup's registers, statistics and apply from one read
    assert fwd(record(golden, 'taxibj_vgg_32')) == ['conv3_band', 'bn_train_fwd_slab']
    # a BatchNorm without running estimates has nothing to fold in the apply launch
    assert fwd(record(golden, 'dcgan_c2', bn='train_untracked'))[2:] == ['bn_stats', 'bn_act_fwd']
    assert fwd(record(golden, 'dcgan_c2'))[2:] == ['bn_stats_ub', 'bn_act_fwd']


def test_epilogue_statistics_are_opt_in_and_replace_the_pass(golden):
    r = record(golden, 'taxibj_vgg_32', sums='1')
    assert fwd(r) == ['bn_sums_buffer', 'conv3_band', 'bn_stats_from_sums_fold', 'bn_act_fwd']
    assert [a.get('reset', True) for n, a in r['forward'] if n == 'bn_stats_from_sums_fold'] == [True]
    assert fwd(record(golden, 'taxibj_vgg_32', sums='parts')) == ['conv3_band_parts', 'bn_stats_from_parts_fold', 'bn_act_fwd']
    assert fwd(record(golden, 'dcgan_c2', sums='1')) == ['space_to_depth2', 'bn_sums_buffer', 'conv_k4s2_gather', 'bn_stats_from_sums_fold', 'bn_act_fwd']
    assert fwd(record(golden, 'dcgan_c2', sums='parts')) == ['space_to_depth2', 'conv3_band_parts', 'bn_stats_from_parts_fold', 'bn_act_fwd']


def test_a_band_layer_small_enough_for_the_one_launch_batchnorm_takes_no_epilogue_statistics(golden):
    for sums in ('', '1', 'parts'):
        assert fwd(record(golden, 'vgg_4x4_wide', sums=sums)) == ['conv3_band', 'bn_train_fwd_small']
    # two call groups of six maps: one launch only with VS_BN_SMALL_GROUPS=1 ...
    assert fwd(record(golden, 'taxibj_vgg_32', g=2, small='1')) == ['conv3_band', 'bn_train_fwd_small']
    # ... but "small" in front of the epilogue forms is judged on the whole batch, so with both switches the epilogue wins
    assert fwd(record(golden, 'taxibj_vgg_32', g=2, small='1', sums='parts')) == ['conv3_band_parts', 'bn_stats_from_parts_fold', 'bn_act_fwd']


def test_sst_integrator_512_to_512_layer_takes_img16_on_8_maps_and_band_on_many(golden):
    r = record(golden, 'sst_res_mid')
    assert fwd(r) == ['conv3_img16', 'bn_train_fwd_small_slabs']
    assert bwd(r) == ['bn_act_bwd', 'conv_wgrad', 'conv3_img16', 'slab_sum']
    assert fwd(record(golden, 'sst_res_mid', bn='none')) == ['conv3_img16', 'slab_sum', 'act_fwd']
    assert fwd(record(golden, 'sst_res_mid', bn='eval')) == ['conv3_img16', 'slab_sum', 'bn_act_fwd']
    # call groups, or more than 32 maps, keep it off the few-maps kernel: the band takes it (k3tap is never reached, see the writer)
    assert G.forward_route(record(golden, 'sst_res_mid', g=2)) == 'band'
    assert fwd(record(golden, 'sst_res_batched')) == ['conv3_band', 'bn_train_fwd_slab']


def test_fp32_always_takes_cols(golden):
    rows = [r for k, r in golden.items() if k.startswith('fp32|')]
    assert rows and {G.forward_route(r) for r in rows} == {'cols'}
    assert {G.dx_route(r) for r in rows} <= {'conv_dgrad', None}


def test_dcgan_encoder_stride_2_layers_keep_the_parity_planes_for_the_weight_gradient(golden):
    r = record(golden, 'dcgan_c2')
    assert fwd(r)[:2] == ['space_to_depth2', 'conv_k4s2_gather']
    assert r['saved'][0] == ['bf16', [6, 256, 16, 16]] and r['x_shape'] == [6, 64, 32, 32]
    assert bwd(r) == ['bn_act_bwd', 'conv_k4s2_wgrad', 'conv_dgrad']
    # 8 x 8 -> 4 x 4 too: the row-band weight gradient serves 4 x 4 planes
    r = record(golden, 'dcgan_c4_8to4')
    assert r['saved'][0] == ['bf16', [18, 256, 4, 4]] and 'conv_k4s2_wgrad' in bwd(r)
    assert fwd(record(golden, 'dcgan_c2', bn='none')) == ['space_to_depth2', 'conv_k4s2_gather', 'act_fwd']


def test_stride_2_layer_with_fewer_than_8_output_channels_gathers_on_planes_but_keeps_x(golden):
    # the row-band weight gradient does not serve Cout < 8: forward on the planes, backward gets x and the column-matrix weight gradient (k4_gather)
    for bn in ('train', 'eval'):
        r = record(golden, 'k4_thin_cout', bn=bn)
        assert G.forward_route(r) == 'k4_gather' and fwd(r)[:2] == ['space_to_depth2', 'conv_k4s2_gather']
        assert r['saved'][0] == ['bf16', [6, 64, 32, 32]] and r['saved'][1] == ['bf16', [6, 4, 16, 16]]
        assert 'conv_wgrad' in bwd(r) and 'conv_k4s2_wgrad' not in bwd(r)
    # no epilogue statistics on this route, whatever the switch says
    for sums in ('1', 'parts'):
        assert fwd(record(golden, 'k4_thin_cout', sums=sums)) == fwd(record(golden, 'k4_thin_cout'))
    # only in front of a BatchNorm
    assert G.forward_route(record(golden, 'k4_thin_cout', bn='none')) == 'cols'


def test_decoder_tap_kernel_carries_its_batchnorm_sums_and_no_reset(golden):
    for layer in ('dcgan_upc2', 'dcgan_upc3', 'dcgan_upc4'):
        r = record(golden, layer)
        assert fwd(r) == ['convt_tap_fwd', 'bn_stats_from_sums_fold', 'bn_act_fwd']
        assert [a.get('reset', True) for n, a in r['forward'] if n == 'bn_stats_from_sums_fold'] == [False]
        assert fwd(record(golden, layer, bn='eval')) == ['convt_tap_fwd', 'bn_act_fwd']
        # its backward: the parity planes of dz serve the weight gradient and the input gradient
        assert bwd(r) == ['bn_act_bwd', 'space_to_depth2', 'conv_k4s2_wgrad', 'conv_k4s2_gather']


def test_tap_without_batchnorm_only_when_the_result_stays_in_the_compute_type(golden):
    assert fwd(record(golden, 'dcgan_upc3', bn='none')) == ['convt_tap_fwd', 'act_fwd']
    assert G.forward_route(record(golden, 'dcgan_upc3', bn='none', o32=1)) == 'cols'


def test_one_launch_small_batchnorm_is_tried_by_band_and_cols_only(golden):
    tried = {G.forward_route(r) for r in golden.values() if 'bn_train_fwd_small' in G.names(r['forward'])}
    assert tried == {'band', 'cols'}


def test_input_gradient_of_a_stride_2_layer_takes_the_tap_kernel_only_for_a_16_bit_input(golden):
    assert G.dx_route(record(golden, 'dcgan_c2', xlowp=1)) == 'tap'
    assert G.dx_route(record(golden, 'dcgan_c2', xlowp=0)) == 'conv_dgrad'


def test_thin_and_odd_layers_take_cols(golden):
    for layer in ('dcgan_c1_thin', 'vgg_first_thin', 'dcgan_upc5_thin', 'dcgan_upc1', 'dcgan_c5_valid', 'chairs_stem', 'k3_odd_24', 'vgg_dec_last'):
        for bn in ('train', 'eval', 'none'):
            assert G.forward_route(record(golden, layer, bn=bn)) == 'cols'
        assert G.dx_route(record(golden, layer)) == 'conv_dgrad'


def test_no_gradient_no_launch(golden):
    r = record(golden, 'taxibj_vgg_32', xg=0, wg=0)
    assert bwd(r) == ['bn_act_bwd'] and r['grad_is_none'] == [True, True, False, False, False]

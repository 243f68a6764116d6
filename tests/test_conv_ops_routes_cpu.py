"""Which C-ABI launches `ops.conv_fwd`, `ops.conv_dgrad` and `ops.conv_wgrad` issue, in which order and with which arguments: every case of
tests/make_golden_conv_ops_routes.py replayed on the CPU and compared EXACTLY with tests/golden/conv_ops_routes.json (the launch names of every
case as text, everything else through a digest of the case's full record; a case that moves is printed in full).

The library is the recording proxy of tests/cabi_recorder.py: the `ops` wrappers themselves run, on CPU tensors, the host-only queries
(`*_supported`, workspace sizes, slab counts) are the real ones, so a row that moves is a call that changed route (or launch order, or an
argument, or which operand piece a term of the fp32 split reads).  The fixture was written by the three functions as they stood before their
route ladders were folded.
"""
import json

import pytest

import make_golden_conv_ops_routes as G


@pytest.fixture(scope='module')
def golden():
    """{key: full record} of every case as the code stands, replayed once for the module."""
    return G.replay()


def test_every_case_replays_the_fixture_exactly(golden):
    with open(G.PATH) as f:
        moved = G.moved(golden, json.load(f))
    for key, what, now, was in moved[:5]:
        print('%s: %s\n  now    %s\n  stored %s\n  full record now: %s' % (key, what, now, was, golden[key]))
    assert not moved, '%d of %d cases moved, e.g. %s' % (len(moved), len(golden), [m[:2] for m in moved[:5]])


def test_the_fixture_reaches_every_route_and_both_fall_throughs(golden):
    seen = G.coverage(golden)
    assert not [label for label in G.REQUIRED if label not in seen]


def test_the_product_of_factors_is_there(golden):
    keys = [k.split('|') for k in golden]
    assert {k[0] for k in keys} == {'bf16', 'fp16', 'fp32'}
    assert {k[1] for k in keys} == {','.join(str(int(v)) for v in g) for g in G.GEOMETRIES}
    assert {k[2] for k in keys} == {'%s:%s' % (op, v) for op, variants in G.CALLS.items() for v in variants}
    for position, values in ((3, {'split=', 'split=1'}), (4, {'cols=', 'cols=0'}), (5, {'band=', 'band=0'})):
        assert {k[position] for k in keys} == values
    assert {k[0] for k in keys if k[3] == 'split=1'} == {'fp32'} and 'fp32' not in {k[0] for k in keys if k[5] == 'band=0'}


# ------------------------------------------------------------------------------------------------------------------ named decisions
def record(golden, geom, op, precision='fp32', split='1', cols='', band=''):
    return golden['%s|%s|%s|split=%s|cols=%s|band=%s' % (precision, ','.join(str(int(v)) for v in geom), op, split, cols, band)]


def operands(r, symbol, positions):
    """The named operands of every `symbol` launch of a record, in order."""
    return [tuple(args[p] for p in positions) for name, args in r['log'] if name == symbol]


TERMS = [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)]


def test_the_six_terms_pair_the_pieces_as_the_summation_order_needs(golden):
    # forward and input gradient: (xs[i], ws[j]), the bias on the first term only
    r = record(golden, (2, 64, 32, 32, 96, 3, 1, 1, False), 'fwd:plain')
    assert operands(r, 'vs_conv3_band_bn', (1, 2, 3)) == [('x.%d' % i, 'pack(w.%d)' % j, 'bias' if n == 0 else 0) for n, (i, j) in enumerate(TERMS)]
    r = record(golden, (16, 64, 32, 32, 64, 4, 2, 1, False), 'dgrad:plain')
    assert operands(r, 'vs_convt_k4s2_tap_fwd_f32', (1, 2, 3)) == [('dy.%d' % i, 'pack(w.%d)' % j, 0) for i, j in TERMS]
    # 3x3 weight gradient: conv_wgrad(ds[j], xs[i]) (arguments: x, dy), chained through `into`
    r = record(golden, (2, 64, 32, 32, 96, 3, 1, 1, False), 'wgrad:into')
    assert operands(r, 'vs_conv3_wgrad_band', (1, 2)) == [('x.%d' % i, 'dy.%d' % j) for i, j in TERMS]
    assert r['result_is'] == 'into' and [a[2:4] for n, a in r['log'] if n == 'vs_conv3_wgrad_band_finish'] == [['into', 'into']] * 6
    # k4s2 weight gradient: (ss[j], planes[i]) (arguments: planes, small map)
    r = record(golden, (16, 64, 32, 32, 64, 4, 2, 1, False), 'wgrad:fresh')
    assert operands(r, 'vs_conv_k4s2_wgrad_band', (1, 2)) == [('planes(x.%d)' % i, 'dy.%d' % j) for i, j in TERMS]
    r = record(golden, (16, 64, 16, 16, 64, 4, 2, 1, True), 'wgrad:fresh')          # (ConvTranspose2d: the large map is dy)
    assert operands(r, 'vs_conv_k4s2_wgrad_band', (1, 2)) == [('planes(dy.%d)' % i, 'x.%d' % j) for i, j in TERMS]
    # thin weight gradient: (bs[i], ss[j])
    r = record(golden, (3, 5, 64, 64, 64, 4, 2, 1, False), 'wgrad:out')
    assert operands(r, 'vs_conv_thin_wgrad', (1, 2)) == [('dy.%d' % i, 'x.%d' % j) for i, j in TERMS]
    assert r['result_is'] == 'out' and [a[5:7] for n, a in r['log'] if n == 'vs_conv_thin_wgrad'] == [[0, 'out']] + [['out', 'out']] * 5


def test_an_unsupported_split_candidate_drops_to_the_next_one_and_then_to_the_plain_ladder(golden):
    # a 3x3 layer with one output channel: past the band to the thin split
    r = record(golden, (2, 64, 64, 64, 1, 3, 1, 1, False), 'fwd:plain')
    assert G.names(r['log']) == ['vs_conv_thin_reduce'] * 6
    # k5 s2 p3: no split family serves it, the fp32 column matrix keeps it
    for op, symbol in (('fwd:plain', 'vs_conv2d_fwd'), ('dgrad:plain', 'vs_conv2d_dgrad'), ('wgrad:fresh', 'vs_conv2d_wgrad_acc')):
        assert G.names(record(golden, (2, 15, 64, 64, 16, 5, 2, 3, False), op)['log'])[-1:] == [symbol]


def test_without_the_switch_fp32_never_takes_a_16_bit_family(golden):
    rows = {k: r for k, r in golden.items() if k.startswith('fp32|') and '|split=|' in k}
    assert rows and not [k for k, r in rows.items() if G.route(k, r)[0]]
    assert {G.route(k, r)[1] for k, r in rows.items()} == {'gemm_1x1', 'gemm_full', 'cols', 'colsT'}

"""Generate tests/golden/conv_block_routes.json: which `ops` launches, in which order and with which arguments, `functional.ConvBlock` issues
forward and backward for a grid of layers, and what it keeps for backward.

TEST INFRASTRUCTURE ONLY; needs the built library, no GPU (the launching `ops` functions are the recording CPU stand-ins of
tests/ops_standins.py, the `*_supported` / `*_enabled` / `band_bn_mode` functions are the real host-only ones):

    python tests/make_golden_conv_block_routes.py

The committed table was written by ConvBlock as it stood BEFORE its forward was split into a route choice, a conv stage and a BatchNorm tail, so
tests/test_conv_block_routes_cpu.py checks that refactor against the old ladder and every later change shows which layers changed route.
Regenerate it only with a change that means to move a decision.

A record = forward log, (dtype, shape) of ctx.saved_tensors, ctx.x_shape, (dtype, shape) of the result, backward log of `y.backward(dy)` with a
dy of the result's dtype, which of the five gradients (x, w, b, gamma, beta) are None.  A log entry = [ops function, {argument name: value}], tensors as [dtype, shape].
An argument left at the default of the real function is not logged.  What of it is stored: see `pack`.
"""
import contextlib
import hashlib
import itertools
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
PATH = os.path.join(HERE, 'golden', 'conv_block_routes.json')

SWITCHES = ('VS_BAND_BN_SUMS', 'VS_BN_SMALL_GROUPS')
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}
# name -> (B, Cin, H, W, Cout, k, stride, pad, transposed): layers of the five workloads at their smallest size and the shapes
# tests/test_conv_gpu.py uses for each kernel family
LAYERS = {
    'dcgan_c1_thin': (6, 5, 64, 64, 64, 4, 2, 1, False),            # Cin < 16: the thin-channel kernels inside conv_fwd
    'dcgan_c2': (6, 64, 32, 32, 128, 4, 2, 1, False),               # planes [6, 256, 16, 16]
    'dcgan_c3': (6, 128, 16, 16, 256, 4, 2, 1, False),              # 8 x 8 planes; its input gradient is on 8 x 8 maps
    'dcgan_c4_8to4': (18, 64, 8, 8, 96, 4, 2, 1, False),            # 8 x 8 -> 4 x 4: the gather without the row-band weight gradient
    'k4_thin_cout': (6, 64, 32, 32, 4, 4, 2, 1, False),             # fewer than 8 output channels: the row-band weight gradient does not serve them
    'dcgan_c5_valid': (6, 128, 4, 4, 64, 4, 1, 0, False),           # 4 x 4 valid -> 1 x 1
    'dcgan_upc1': (6, 148, 1, 1, 512, 4, 1, 0, True),               # ConvTranspose2d k4 s1 p0: 1 x 1 -> 4 x 4
    'dcgan_upc2': (16, 512, 4, 4, 256, 4, 2, 1, True),               # ConvTranspose2d k4 s2 p1 on 4 x 4 maps
    'dcgan_upc3': (8, 128, 8, 8, 64, 4, 2, 1, True),                # ... on 8 x 8 maps
    'dcgan_upc4': (16, 64, 16, 16, 64, 4, 2, 1, True),              # ... on 16 x 16 maps: the output gradient has 32 x 32 maps
    'dcgan_upc5_thin': (6, 64, 32, 32, 1, 4, 2, 1, True),           # one output channel
    'taxibj_vgg_32': (12, 64, 32, 32, 64, 3, 1, 1, False),           # the TaxiBJ 32 x 32 3 x 3 layers: too many maps for the one-launch BatchNorm, six per call group
    'vgg_4x4_wide': (16, 512, 4, 4, 512, 3, 1, 1, False),           # the VGG encoders' 512-channel layers
    'vgg_first_thin': (4, 8, 32, 32, 64, 3, 1, 1, False),           # Cin < 16
    'vgg_dec_last': (2, 64, 32, 32, 2, 3, 1, 1, True),              # ConvTranspose2d k3 s1 p1
    'sst_res_mid': (8, 512, 16, 16, 512, 3, 1, 1, False),           # the SST integrator's 512 -> 512 layer on 8 maps
    'sst_res_batched': (34, 512, 16, 16, 512, 3, 1, 1, False),      # 512 -> 512 on more than 32 maps
    'sst_img_b32': (32, 64, 16, 16, 33, 3, 1, 1, False),            # the largest batch of the few-maps kernel
    'k3_odd_24': (4, 72, 24, 24, 64, 3, 1, 1, False),               # rows of 24 pixels: no row-band kernel
    'chairs_stem': (2, 15, 64, 64, 16, 5, 2, 3, False),             # k5 s2 p3
}
FEW = ('dcgan_c2', 'dcgan_upc3', 'taxibj_vgg_32', 'sst_res_mid', 'dcgan_upc1', 'chairs_stem')      # the layers fp16 and fp32 run


@contextlib.contextmanager
def switches(env):
    """The ConvBlock switches set to exactly `env` (they are read per call); the caller's values come back afterwards."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def case_keys():
    """Every case as a dict of its factors.  bf16 runs every layer, fp16 and fp32 the layers of FEW.  Thinned where a factor cannot matter: the two
    switches only select something in the forward behind a training-mode BatchNorm, so their settings run with every BatchNorm-training layer,
    group count and `out_fp32` in bf16 but with both gradients wanted and an fp32 input only; a 16-bit input only matters to the input gradient."""
    for precision in DTYPES:
        for layer in (LAYERS if precision == 'bf16' else FEW):
            for bn, groups, out_fp32 in itertools.product(('train', 'eval', 'none'), (1, 2), (False, True)):
                base = dict(precision=precision, layer=layer, bn=bn, groups=groups, out_fp32=out_fp32, sums='', small='')
                for x_lowp, x_grad, w_grad in ((False, True, True), (False, True, False), (False, False, True), (False, False, False),
                                               (True, True, True), (True, True, False)):
                    if not (x_lowp and precision == 'fp32'):
                        yield dict(base, x_lowp=x_lowp, x_grad=x_grad, w_grad=w_grad)
                if bn == 'train' and layer in FEW:
                    yield dict(base, bn='train_untracked', x_lowp=False, x_grad=True, w_grad=True)      # (a BatchNorm without running estimates)
                if bn == 'train' and precision == 'bf16':
                    for sums, small in list(itertools.product(('', '1', 'parts'), ('', '1')))[1:]:
                        yield dict(base, x_lowp=False, x_grad=True, w_grad=True, sums=sums, small=small)


def key_of(c):
    return '%s|%s|bn=%s|g=%d|o32=%d|xlowp=%d|xg=%d|wg=%d|sums=%s|small=%s' % (
        c['precision'], c['layer'], c['bn'], c['groups'], c['out_fp32'], c['x_lowp'], c['x_grad'], c['w_grad'], c['sums'], c['small'])


def run_case(c, monkeypatch):
    """One ConvBlock forward + backward of case `c` under fresh stand-ins -> its record."""
    from ops_standins import StandIns, describe
    from spatiotemporal_variable_separation_amd import functional as VF
    rec = StandIns()
    rec.install(monkeypatch)
    rec.install_launches(monkeypatch)
    B, Cin, H, W, Cout, k, stride, pad, transposed = LAYERS[c['layer']]
    cdt = DTYPES[c['precision']]
    x = torch.zeros((B, Cin, H, W), dtype=cdt if c['x_lowp'] else torch.float32, requires_grad=c['x_grad'])
    w = torch.nn.Parameter(torch.zeros((Cin, Cout, k, k) if transposed else (Cout, Cin, k, k)), requires_grad=c['w_grad'])
    b = torch.nn.Parameter(torch.zeros(Cout))
    has_bn = c['bn'] != 'none'
    gamma, beta = (torch.nn.Parameter(torch.ones(Cout)), torch.nn.Parameter(torch.zeros(Cout))) if has_bn else (None, None)
    rmean, rvar = (torch.zeros(Cout), torch.ones(Cout)) if c['bn'] in ('train', 'eval') else (None, None)
    cfg = (transposed, stride, pad, has_bn, 'leaky_relu', c['bn'].startswith('train'), 0.1, 1e-5, c['out_fp32'], c['groups'])
    env = {k_: v for k_, v in (('VS_BAND_BN_SUMS', c['sums']), ('VS_BN_SMALL_GROUPS', c['small'])) if v}
    with switches(env), VF.precision(c['precision']):
        y = VF.ConvBlock.apply(x, w, b, gamma, beta, rmean, rvar, cfg)
        forward, ctx = list(rec.log), y.grad_fn
        saved, x_shape = [describe(t) for t in ctx.saved_tensors], list(ctx.x_shape)
        del rec.log[:]
        y.backward(torch.empty_like(y))
    return {'forward': forward, 'saved': saved, 'x_shape': x_shape, 'result': describe(y),
            'backward': list(rec.log), 'grad_is_none': [t is None or t.grad is None for t in (x, w, b, gamma, beta)]}


def names(log):
    return [entry[0] for entry in log]


def forward_route(record):
    """The forward route of a record, read off its log (the launch that convolves)."""
    f = names(record['forward'])
    if 'space_to_depth2' in f:
        return 'k4_planes' if record['saved'][0][1][1] != record['x_shape'][1] else 'k4_gather'
    for launch, route in (('conv3_img16', 'img16'), ('conv3_band', 'band'), ('conv3_band_parts', 'band'), ('convt_tap_fwd', 'tap'),
                          ('conv_k3_tap_fwd', 'k3tap'), ('conv_fwd', 'cols')):
        if launch in f:
            return route
    raise AssertionError(f)


def dx_route(record):
    """The input-gradient route of a record (None: no input gradient)."""
    for name, args in record['backward']:
        if args.get('role') == 'dgrad':
            return {'conv_k4s2_gather': 'dz_planes', 'convt_tap_fwd': 'tap', 'conv3_img16': 'img16', 'conv3_band': 'band', 'conv_k3_tap_fwd': 'k3tap'}[name]
        if name == 'conv_dgrad':
            return 'conv_dgrad'
    return None


def coverage(records):
    """What {key: record} reaches, as a set of labels; REQUIRED lists what it must reach."""
    seen = set()
    for key, r in records.items():
        f, bwd = names(r['forward']), names(r['backward'])
        bn = key.split('|')[2][3:].replace('_untracked', '')
        route = forward_route(r)
        seen.add('fwd:%s:%s' % (route, bn))
        if 'bn_stats_from_sums_fold' in f and route in ('band', 'k4_planes'):
            seen.add('epilogue:sums:%s' % route)
        if 'bn_stats_from_parts_fold' in f:
            seen.add('epilogue:parts:%s' % route)
        for launch in ('bn_train_fwd_small_slabs', 'bn_train_fwd_small', 'bn_train_fwd_slab', 'bn_stats_ub', 'bn_stats'):
            if launch in f:
                seen.add('tail:%s' % launch)
        if bn == 'eval':
            seen.add('tail:eval')
        if dx_route(r):
            seen.add('dx:%s' % dx_route(r))
        if 'conv_k4s2_wgrad' in bwd:
            seen.add('k4_wgrad:%s' % ('planes_of_dz' if 'space_to_depth2' in bwd else 'planes_kept'))
    return seen


# NOT reachable with the real `*_supported` functions, so absent: k3tap, forward and input gradient (conv3_img16_supported or conv3_band_supported
# answer yes wherever conv_k3_tap_supported does: the band serves every 4x4 / 8x8 / 16x16 map with Cin >= 384 and Cout >= 256)
REQUIRED = (['fwd:%s:train' % r for r in ('k4_planes', 'k4_gather', 'img16', 'band', 'tap', 'cols')] + ['fwd:k4_gather:eval']
            + ['fwd:%s:none' % r for r in ('k4_planes', 'img16', 'band', 'tap', 'cols')]
            + ['epilogue:sums:band', 'epilogue:parts:band', 'epilogue:sums:k4_planes', 'epilogue:parts:k4_planes',
               'tail:bn_train_fwd_small_slabs', 'tail:bn_train_fwd_small', 'tail:eval']
            + ['dx:%s' % r for r in ('dz_planes', 'tap', 'img16', 'band', 'conv_dgrad')]
            + ['k4_wgrad:planes_kept', 'k4_wgrad:planes_of_dz'])


def pack(records):
    """{key: full record} -> the stored form, small enough to read: per case the NAMES of the launches, forward and backward, which gradients
    are None, and the first 40 bits of the SHA-256 of the full record (arguments, shapes, dtypes, saved tensors, result).  Everything is kept
    once and referred to by index: `logs` = the distinct name lists, `records` = the distinct [forward log, backward log, None-gradients as a
    bit mask, digest], `cases` = the record of every case in the order of `case_keys()`."""
    tables = {name: ([], {}) for name in ('logs', 'records')}

    def intern(name, value):
        items, index = tables[name]
        text = json.dumps(value)
        if text not in index:
            index[text] = len(items)
            items.append(value)
        return index[text]

    cases = []
    for r in records.values():
        mask = sum(1 << i for i, flag in enumerate(r['grad_is_none']) if flag)
        digest = hashlib.sha256(json.dumps(r, separators=(',', ':'), sort_keys=True).encode()).hexdigest()[:10]
        cases.append(intern('records', [intern('logs', names(r['forward'])), intern('logs', names(r['backward'])), mask, digest]))
    return {'logs': tables['logs'][0], 'records': tables['records'][0], 'cases': cases}


def moved(records, stored):
    """The cases of {key: full record} that differ from the stored form: [(key, what differs, now, stored)]."""
    now, out = pack(records), []
    assert len(now['cases']) == len(stored['cases']), (len(now['cases']), len(stored['cases']))
    for key, i, j in zip(records, now['cases'], stored['cases']):
        n, w = now['records'][i], stored['records'][j]
        for what, a, b in (('forward launches', now['logs'][n[0]], stored['logs'][w[0]]), ('backward launches', now['logs'][n[1]], stored['logs'][w[1]]),
                           ('None gradients', n[2], w[2]), ('arguments, shapes, dtypes or what is kept (digest)', n[3], w[3])):
            if a != b:
                out.append((key, what, a, b))
                break
    return out


def replay():
    """{key: record} of every case, as the code stands."""
    import pytest
    records = {}
    for c in case_keys():
        monkeypatch = pytest.MonkeyPatch()
        try:
            records[key_of(c)] = json.loads(json.dumps(run_case(c, monkeypatch)))
        finally:
            monkeypatch.undo()
    return records


def main():
    from spatiotemporal_variable_separation_amd import _lib
    _lib.build_library()
    records = replay()
    missing = [label for label in REQUIRED if label not in coverage(records)]
    assert not missing, missing
    stored = pack(records)
    dump = lambda v: json.dumps(v, separators=(',', ':'))
    rows = lambda items, n: ',\n'.join(','.join(dump(v) for v in items[i:i + n]) for i in range(0, len(items), n))
    with open(PATH, 'w') as f:
        f.write('{"logs":[\n%s\n],\n"records":[\n%s\n],\n"cases":[\n%s\n]}\n' % (rows(stored['logs'], 1), rows(stored['records'], 8), rows(stored['cases'], 48)))
    print('wrote', PATH, len(records), 'cases,', len(stored['records']), 'distinct records,', os.path.getsize(PATH), 'bytes')
    print(sorted(coverage(records)))


if __name__ == '__main__':
    main()

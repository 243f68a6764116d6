"""Generate tests/golden/conv_ops_routes.json: which C-ABI launches, in which order and with which arguments, `ops.conv_fwd`, `ops.conv_dgrad` and
`ops.conv_wgrad` issue for a grid of geometries, dtypes and switches.

TEST INFRASTRUCTURE ONLY; needs the built library, no GPU (the library is the recording proxy of tests/cabi_recorder.py: the host-only queries
are the real ones, every launch is logged, the `ops` wrappers themselves run on CPU tensors):

    python tests/make_golden_conv_ops_routes.py

The committed table was written by the three functions as they stood BEFORE their route ladders were folded into one geometry, one plain route
choice, one split route choice and one six-term driver, so tests/test_conv_ops_routes_cpu.py checks that refactor against the old ladders and
every later change shows which calls changed route.  Regenerate it only with a change that means to move a decision.

A record = the ordered log ([symbol, arguments]: scalars as they are, pointers as names, see cabi_recorder), (dtype, shape) of the result and
whether the result IS `into` or `out`.  What of it is stored: see `pack` (the form of tests/golden/conv_block_routes.json).
"""
import contextlib
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
PATH = os.path.join(HERE, 'golden', 'conv_ops_routes.json')

from make_golden_conv_block_routes import DTYPES, LAYERS          # noqa: E402
from test_conv_gpu import GEOMS, SPLIT_GEOMS, THIN_GEOMS           # noqa: E402

SWITCHES = ('VARSEP_FP32_SPLIT', 'VS_CONV_COLS', 'VS_CONV_WGRAD_BAND')
# (B, Cin, H, W, Cout, k, stride, pad, transposed), each once, in the order of the four lists
GEOMETRIES = list(dict.fromkeys(list(GEOMS) + list(THIN_GEOMS) + list(LAYERS.values()) + [g for g, _ in SPLIT_GEOMS]))
CALLS = {'fwd': ('plain', 'w_packed'), 'dgrad': ('plain', 'w_packed', 'cols_from_wgrad'), 'wgrad': ('fresh', 'into', 'out')}


@contextlib.contextmanager
def switches(env):
    """The three switches set to exactly `env` (they are read per call); the caller's values come back afterwards."""
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
    """Every case as a dict of its factors: geometry x precision x switches x (op, variant).  Thinned where a factor cannot matter:
      * VARSEP_FP32_SPLIT=1 runs fp32 only (the predicate asks for fp32 operands);
      * VS_CONV_WGRAD_BAND=0 is read by `conv3_wgrad_band_supported` alone and that answers no for fp32 anyway: 16-bit weight gradients of
        Conv2d k3 s1 p1 only;
      * VS_CONV_COLS=0 is read by `_conv_workspace` alone, after the route is chosen: it runs with the default variant of each op, without the
        split, in fp32 and bf16;
      * a `w_packed` given is only looked at by the form that consumes one (ConvTranspose2d forward, Conv2d input gradient), and
        `cols_from_wgrad` only by the ConvTranspose2d input gradient."""
    for geom in GEOMETRIES:
        k, stride, pad, transposed = geom[5:]
        for precision in DTYPES:
            for split in (('', '1') if precision == 'fp32' else ('',)):
                for op, variants in CALLS.items():
                    for variant in variants:
                        if variant == 'w_packed' and transposed != (op == 'fwd'):
                            continue
                        if variant == 'cols_from_wgrad' and not transposed:
                            continue
                        base = dict(geom=geom, precision=precision, op=op, variant=variant, split=split, cols='', band='')
                        yield base
                        if variant in ('plain', 'fresh') and not split and precision != 'fp16':
                            yield dict(base, cols='0')
                        if op == 'wgrad' and precision != 'fp32' and (k, stride, pad, transposed) == (3, 1, 1, False):
                            yield dict(base, band='0')


def key_of(c):
    return '%s|%s|%s:%s|split=%s|cols=%s|band=%s' % (c['precision'], ','.join(str(int(v)) for v in c['geom']), c['op'], c['variant'],
                                                     c['split'], c['cols'], c['band'])


_TENSORS = {}


def _tensor(role, shape, dtype):
    """The case tensors, made once per (role, shape, dtype): no launch runs, so nothing ever writes to them."""
    key = (role, tuple(shape), dtype)
    if key not in _TENSORS:
        _TENSORS[key] = torch.zeros(tuple(shape), dtype=dtype)
    return _TENSORS[key]


def run_case(c, monkeypatch):
    """One call of case `c` under a fresh recorder -> its record."""
    from cabi_recorder import Recorder
    from ops_standins import describe
    from spatiotemporal_variable_separation_amd import _lib, ops
    B, Cin, H, W, Cout, k, stride, pad, transposed = c['geom']
    dt = DTYPES[c['precision']]
    OH, OW = ops._conv_out_hw(H, W, k, stride, pad, transposed)
    w_shape = (Cin, Cout, k, k) if transposed else (Cout, Cin, k, k)
    rec = Recorder()
    rec.install(monkeypatch)
    x, w, dy = (rec.name(n, _tensor(n, s, dt)) for n, s in (('x', (B, Cin, H, W)), ('w', w_shape), ('dy', (B, Cout, OH, OW))))
    bias = rec.name('bias', _tensor('bias', (Cout,), torch.float32))
    w_packed = None
    if c['variant'] == 'w_packed':
        w_packed = rec.name('w_packed', _tensor('w_packed', (_lib.load_library().vs_conv_packed_elems(w_shape[0], w_shape[1], k, k, stride, pad),), dt))
    into = rec.name('into', _tensor('into', w_shape, torch.float32)) if c['variant'] == 'into' else None
    out = rec.name('out', _tensor('out', w_shape, torch.float32)) if c['variant'] == 'out' else None
    env = {k_: v for k_, v in (('VARSEP_FP32_SPLIT', c['split']), ('VS_CONV_COLS', c['cols']), ('VS_CONV_WGRAD_BAND', c['band'])) if v}
    with switches(env):
        if c['op'] == 'fwd':
            r = ops.conv_fwd(x, w, bias, stride, pad, transposed, torch.float32, w_packed=w_packed)
        elif c['op'] == 'dgrad':
            r = ops.conv_dgrad(dy, w, (B, Cin, H, W), stride, pad, transposed, torch.float32, w_packed=w_packed,
                               cols_from_wgrad=c['variant'] == 'cols_from_wgrad')
        else:
            r = ops.conv_wgrad(dy, x, w_shape, stride, pad, transposed, into=into, out=out)
    return {'log': rec.log, 'result': describe(r), 'result_is': 'into' if r is into else ('out' if r is out else None)}


def names(log):
    return [entry[0] for entry in log]


_FAMILY = (('vs_conv3_band_bn', 'conv3:band'), ('vs_conv3_img16', 'conv3:img16'), ('vs_conv_k4s2_band_bn', 'k4s2_gather'), ('vs_convt_k4s2_tap_fwd_f32', 'tap'),
           ('vs_conv_k4s2_wgrad_band', 'k4s2_wgrad'), ('vs_conv3_wgrad_band', 'band_wgrad'), ('vs_conv_thin_expand', 'thin:expand'),
           ('vs_conv_thin_reduce', 'thin:reduce'), ('vs_conv_thin_wgrad', 'thin:wgrad'), ('vs_gemm', 'gemm'), ('vs_conv2d_fwd', 'cols'),
           ('vs_conv2d_dgrad', 'cols'), ('vs_conv2d_wgrad_acc', 'cols'), ('vs_conv_transpose2d_fwd', 'colsT'), ('vs_conv_transpose2d_dgrad', 'colsT'),
           ('vs_conv_transpose2d_wgrad_acc', 'colsT'))


def route(key, record):
    """(six launches or one, the route) of a record, read off its log."""
    log = record['log']
    for symbol, label in _FAMILY:
        hits = [args for name, args in log if name == symbol]
        if hits:
            assert len(hits) in (1, 6), (key, symbol, len(hits))
            if label == 'thin:wgrad':           # (arguments: type code, the many-channel map, the thin one, ...)
                label += '_big_dy' if str(hits[0][1]).startswith('dy') else '_big_x'
            if label == 'gemm':
                label += '_1x1' if key.split('|')[1].endswith(',1') else '_full'
            return len(hits) == 6, label
    raise AssertionError((key, names(log)))


def coverage(records):
    """What {key: record} reaches, as a set of labels; REQUIRED lists what it must reach."""
    seen = set()
    for key, r in records.items():
        op = key.split('|')[2].split(':')[0]
        geom = [int(v) for v in key.split('|')[1].split(',')]
        six, label = route(key, r)
        seen.add('%s:%s:%s' % ('split' if six else 'plain', op, label))
        if 'split=1' in key:
            if not six:
                seen.add('fall:to_plain:%s' % label)
            elif geom[5:] == [3, 1, 1, 0] and label.startswith('thin'):
                seen.add('fall:past_the_band_to:%s' % label)
    return seen


# every route an op has, plain and under the split, and both kinds of fall-through: a split candidate that answers "unsupported" drops to the NEXT
# split candidate (a 3 x 3 layer with one output channel: past the band to the thin split), the last one to the plain ladder (the k5 s2 p3 stem).
# Routes an op does not have: the input gradient never reduces (thin:reduce) and only the weight gradient has band_wgrad / k4s2_wgrad.
REQUIRED = (['plain:%s:%s' % (op, r) for op in CALLS for r in ('gemm_1x1', 'gemm_full', 'cols', 'colsT')]
            + ['plain:fwd:thin:expand', 'plain:fwd:thin:reduce', 'plain:dgrad:thin:expand', 'plain:wgrad:thin:wgrad_big_dy', 'plain:wgrad:thin:wgrad_big_x',
               'plain:wgrad:band_wgrad']
            + ['split:%s:%s' % (op, r) for op in ('fwd', 'dgrad') for r in ('conv3:band', 'conv3:img16', 'k4s2_gather', 'tap', 'thin:expand')]
            + ['split:fwd:thin:reduce', 'split:wgrad:band_wgrad', 'split:wgrad:k4s2_wgrad', 'split:wgrad:thin:wgrad_big_dy', 'split:wgrad:thin:wgrad_big_x']
            + ['fall:past_the_band_to:thin:reduce', 'fall:to_plain:cols', 'fall:to_plain:colsT'])


def pack(records):
    """{key: full record} -> the stored form: `logs` = the distinct launch-name lists, `records` = the distinct [log, 'into' / 'out' / None, first
    40 bits of the SHA-256 of the full record], `cases` = the record of every case in the order of `case_keys()`."""
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
        digest = hashlib.sha256(json.dumps(r, separators=(',', ':'), sort_keys=True).encode()).hexdigest()[:10]
        cases.append(intern('records', [intern('logs', names(r['log'])), r['result_is'], digest]))
    return {'logs': tables['logs'][0], 'records': tables['records'][0], 'cases': cases}


def moved(records, stored):
    """The cases of {key: full record} that differ from the stored form: [(key, what differs, now, stored)]."""
    now, out = pack(records), []
    assert len(now['cases']) == len(stored['cases']), (len(now['cases']), len(stored['cases']))
    for key, i, j in zip(records, now['cases'], stored['cases']):
        n, w = now['records'][i], stored['records'][j]
        for what, a, b in (('launches', now['logs'][n[0]], stored['logs'][w[0]]), ('which tensor the result is', n[1], w[1]),
                           ('arguments, operand names, result dtype or shape (digest)', n[2], w[2])):
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

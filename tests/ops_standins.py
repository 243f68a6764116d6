"""CPU stand-ins for `ops` functions (a plain helper module: tests import it).

`StandIns` replaces the cast / pack functions the derived-copy caches call (tests/test_weight_cache_cpu.py) and the launching functions
`functional.ConvBlock` reaches (tests/test_conv_block_routes_cpu.py): every stand-in returns CPU tensors of the shapes and dtypes the real
wrapper documents and records its call.  The `*_supported`, `*_enabled` and `band_bn_mode` functions stay real (host-only calls into the built
library, which loads without a GPU)."""
import inspect
import weakref

import torch

from spatiotemporal_variable_separation_amd import _lib, ops

F32, F64 = torch.float32, torch.float64


def describe(v):
    """What the log keeps of an argument: a tensor's dtype and shape, scalars as they are, containers element by element."""
    if isinstance(v, torch.Tensor):
        return [describe(v.dtype), list(v.shape)]
    if isinstance(v, torch.dtype):
        return {torch.bfloat16: 'bf16', torch.float16: 'f16', torch.float32: 'f32', torch.float64: 'f64'}[v]
    if isinstance(v, (tuple, list, torch.Size)):
        return [describe(e) for e in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return str(v)


# name -> (arguments by name) -> the tensors the real wrapper returns (uninitialised); shapes as documented in ops.py
def _conv_fwd(a):
    x, w = a['x'], a['w']
    oh, ow = ops._conv_out_hw(x.shape[2], x.shape[3], w.shape[2], a['stride'], a['pad'], a['transposed'])
    return torch.empty((x.shape[0], w.shape[1] if a['transposed'] else w.shape[0], oh, ow), dtype=a['out_dtype'])


def _band_parts(a):
    B, _, H, W = a['x'].shape
    rows = _lib.load_library().vs_conv3_band_bn_parts_rows(B, H, W)
    return torch.empty((B, a['Cout'], H, W), dtype=a['out_dtype']), torch.empty((rows, a['Cout'], 2), dtype=F32)


def _img16(a):
    B, Cin, H, W = a['x'].shape
    return torch.empty((_lib.load_library().vs_conv3_img16_splits(B, Cin, a['Cout']), B, a['Cout'], H, W), dtype=F32)


def _tap(a, scale):
    B, _, H, W = a['x'].shape
    y = torch.empty((B, a['Cout'], scale * H, scale * W), dtype=a.get('out_dtype', a['x'].dtype))
    return y, (torch.empty((a['groups'], a['Cout'], 2), dtype=F64) if a['want_sums'] else None)


def _stats(n):
    return lambda a: tuple(torch.empty((a['groups'], a['x'].shape[1]), dtype=F32) for _ in range(n))


def _bn_small(a):
    x = a['x']
    return (torch.empty(x.shape, dtype=a['out_dtype']),) + tuple(torch.empty((a['groups'], x.shape[1]), dtype=F32) for _ in range(2))


def _bn_small_slabs(a):
    assert a['skip'] is None
    shape, C = a['slabs'].shape[1:], a['slabs'].shape[2]
    return torch.empty(shape, dtype=a['out_dtype']), torch.empty(shape, dtype=a['z_dtype']), torch.empty((1, C), dtype=F32), torch.empty((1, C), dtype=F32)


def _wgrad(a):
    for given in (a['into'], a['out']):
        if given is not None:
            return given
    return torch.empty(tuple(a['w_shape']), dtype=F32)


LAUNCHES = {
    'space_to_depth2': lambda a: torch.empty((a['x'].shape[0], 4 * a['x'].shape[1], a['x'].shape[2] // 2, a['x'].shape[3] // 2), dtype=a['x'].dtype),
    'conv_k4s2_gather': lambda a: torch.empty((a['planes'].shape[0], a['M']) + tuple(a['planes'].shape[2:]), dtype=a['out_dtype']),
    'conv3_band': lambda a: torch.empty((a['x'].shape[0], a['Cout']) + tuple(a['x'].shape[2:]), dtype=a['out_dtype']),
    'conv3_band_parts': _band_parts,
    'conv3_img16': _img16,
    'slab_sum': lambda a: torch.empty(a['slabs'].shape[1:], dtype=a['out_dtype']),
    'convt_tap_fwd': lambda a: _tap(a, 2),
    'conv_k3_tap_fwd': lambda a: _tap(a, 1),
    'conv_fwd': _conv_fwd,
    'act_fwd': lambda a: a['out'] if a['out'] is not None else torch.empty(a['x'].shape, dtype=a['out_dtype'] or a['x'].dtype),
    'bn_stats': _stats(2),
    'bn_stats_ub': _stats(3),
    'bn_act_fwd': lambda a: torch.empty(a['x'].shape, dtype=a['out_dtype']),
    'bn_train_fwd_small': _bn_small,
    'bn_train_fwd_slab': _bn_small,
    'bn_train_fwd_small_slabs': _bn_small_slabs,
    'bn_stats_from_sums_fold': lambda a: tuple(torch.empty(a['sums'].shape[:2], dtype=F32) for _ in range(2)),
    'bn_stats_from_parts_fold': lambda a: tuple(torch.empty((a['groups'], a['parts'].shape[1]), dtype=F32) for _ in range(2)),
    'bn_sums_buffer': lambda a: torch.empty((a['groups'], a['C'], 2), dtype=F64),
    'bn_act_bwd': lambda a: (torch.empty(a['x'].shape, dtype=a['out_dtype']), torch.empty(a['x'].shape[1], dtype=F32), torch.empty(a['x'].shape[1], dtype=F32)),
    'act_bwd': lambda a: torch.empty(a['dy'].shape, dtype=a['out_dtype'] or a['dy'].dtype),
    'chan_sum': lambda a: torch.empty(a['x'].shape[1], dtype=F32),
    'conv_dgrad': lambda a: torch.empty(tuple(a['x_shape']), dtype=a['out_dtype']),
    'conv_wgrad': _wgrad,
    'conv_k4s2_wgrad': _wgrad,
}
UNLOGGED = {'bn_sums_buffer': ('key',)}       # (an address: it names the call site, it is no decision)
SIGNATURES = {name: inspect.signature(getattr(ops, name)) for name in LAUNCHES}         # (of the real functions: taken before any is replaced)


class StandIns:
    """CPU versions of the nine `ops` functions the caches call and of the launching functions ConvBlock reaches.
    `calls`: (name, source tensor, extra arguments, the `out` given) of the cast / pack functions; the batched ones log (name, [(source, flag,
    out given)]).  `made`: weak references to every buffer a cast / pack stand-in allocated.
    `log`: [name, {argument name: `describe`d value}] of EVERY stand-in call in order, arguments bound by name (so a keyword spelled
    positionally is the same entry); an argument left at, or given, the real function's default is not logged."""

    def __init__(self):
        self.calls, self.made, self.log = [], [], []

    def _new(self, shape, dtype):
        buf = torch.empty(shape, dtype=dtype)
        self.made.append(weakref.ref(buf))
        return buf

    def live(self):
        return sum(r() is not None for r in self.made)

    def cast(self, src, dtype, out=None):
        self.calls.append(('cast', src, (dtype,), out))
        self.log.append(['cast', {'src': describe(src), 'dtype': describe(dtype)}])
        buf = self._new(src.shape, dtype) if out is None else out
        return buf.copy_(src)

    def _pack(self, name, w, dtype, extra, out):
        self.calls.append((name, w, (dtype,) + extra, out))
        self.log.append([name, {'w': describe(w), 'dtype': describe(dtype), 'extra': describe(extra)}])
        buf = self._new((w.numel(),), dtype) if out is None else out
        return buf.copy_(w.reshape(-1) * (-1 if extra and extra[0] is True else 1))       # (a flipped / transposed pack differs)

    def _packs(self, name, jobs, dtype):
        self.calls.append((name, [tuple(j) for j in jobs]))
        return [(self._new((w.numel(),), dtype) if out is None else out).copy_(w.reshape(-1) * (-1 if flag else 1)) for w, flag, out in jobs]

    def _launch(self, name):
        signature, result = SIGNATURES[name], LAUNCHES[name]
        default = {k: p.default for k, p in signature.parameters.items() if p.default is not p.empty and k not in UNLOGGED.get(name, ())}
        required = [k for k in signature.parameters if k not in default and k not in UNLOGGED.get(name, ())]

        def stand_in(*args, **kwargs):
            bound = signature.bind(*args, **kwargs)
            bound.apply_defaults()
            a = dict(bound.arguments)
            args = {k: describe(a[k]) for k in required}
            args.update({k: describe(a[k]) for k, d in default.items() if not (a[k] is d or (type(a[k]) is type(d) and a[k] == d))})
            self.log.append([name, args])
            return result(a)
        return stand_in

    def install(self, monkeypatch):
        monkeypatch.setattr(ops, 'cast', self.cast)
        monkeypatch.setattr(ops, 'pack_rollout_weight', lambda w, dtype, transpose, out=None: self._pack('pack_rollout_weight', w, dtype, (bool(transpose),), out))
        monkeypatch.setattr(ops, 'pack_rollout_weights', lambda jobs, dtype: self._packs('pack_rollout_weights', jobs, dtype))
        monkeypatch.setattr(ops, 'conv_pack_weight', lambda w, dtype, stride, pad, out=None: self._pack('conv_pack_weight', w, dtype, (stride, pad), out))
        monkeypatch.setattr(ops, 'convt_tap_pack_weight', lambda w, dtype, out=None: self._pack('convt_tap_pack_weight', w, dtype, (), out))
        monkeypatch.setattr(ops, 'conv_k3_tap_pack_weight', lambda w, dtype, flip, out=None: self._pack('conv_k3_tap_pack_weight', w, dtype, (bool(flip),), out))
        monkeypatch.setattr(ops, 'conv_k4s2_pack_weight', lambda w, dtype, out=None: self._pack('conv_k4s2_pack_weight', w, dtype, (), out))
        monkeypatch.setattr(ops, 'conv3_img16_pack_weight', lambda w, dtype, flip, out=None: self._pack('conv3_img16_pack_weight', w, dtype, (bool(flip),), out))
        monkeypatch.setattr(ops, 'conv3_img16_pack_weights', lambda jobs, dtype: self._packs('conv3_img16_pack_weights', jobs, dtype))

    def install_launches(self, monkeypatch):
        """Additionally: the launching functions of LAUNCHES, and `functional.require_cuda` as a no-op."""
        from spatiotemporal_variable_separation_amd import functional
        for name in LAUNCHES:
            monkeypatch.setattr(ops, name, self._launch(name))
        monkeypatch.setattr(functional, 'require_cuda', lambda *tensors: None)

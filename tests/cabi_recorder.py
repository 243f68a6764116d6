"""A recorder at the C ABI (a plain helper module: tests import it).

`Recorder` stands in for the loaded library: the host-only symbols (`*_supported`, `*_bytes`, `*_elems`, `*_slabs`, `*_rows`, `*_splits`,
`vs_version`, `vs_last_error`, `vs_gemm_plan`) go to the real library, which loads without a GPU; every other symbol -- a launch -- is logged as
[name, arguments] and returns 0.  With `ops.require_cuda`, `ops.stream_ptr` and `ops._workspace` replaced by CPU versions the `ops` wrappers run
to the end on CPU tensors, so the log is the route a call takes THROUGH `ops`, not around it (tests/ops_standins.py replaces the wrappers).

Arguments: scalars as they are, the trailing stream dropped, pointers as NAMES -- a pointer into a tensor given to `name` carries that name,
0 stays 0, anything else is 'tmp'; a pointer array is logged element by element.  Three things hand a name on:
  * `ops._split16` of a named tensor names its pieces `x.0`, `x.1`, `x.2`;
  * a dtype / layout copy of such a piece (`p.float().contiguous()`) keeps the piece's name;
  * an `ops.*pack_weight` call on a named source names its result `pack(<source>)`, `ops.space_to_depth2` its result `planes(<source>)`.
So the log shows the (i, j) order of the six fp32-split terms and which operand carries which index.
"""
import ctypes

import torch

from spatiotemporal_variable_separation_amd import _lib, ops

HOST_SUFFIXES = ('_supported', '_bytes', '_elems', '_slabs', '_rows', '_splits')
HOST_NAMES = ('vs_version', 'vs_last_error', 'vs_gemm_plan')


class _Piece(torch.Tensor):
    """A `_split16` piece: its `.float()` / `.contiguous()` / `.to()` copies take its name in the recorder that made it."""
    recorder = None

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        out = super().__torch_function__(func, types, args, kwargs or {})
        rec = cls.recorder
        if rec is not None and getattr(func, '__name__', '') in ('float', 'contiguous', 'to') and isinstance(out, torch.Tensor):
            name = rec.name_of(args[0].data_ptr())
            if name not in (0, 'tmp'):
                rec.name(name, out)
        return out


class Recorder:
    def __init__(self):
        self.real = _lib.load_library()
        self.log, self.spans, self.keep = [], [], []

    def name(self, name, t):
        """Pointers into `t` are logged as `name` from here on (`t` is kept alive, so its addresses are not handed out again)."""
        if t is not None:
            self.spans.append((t.data_ptr(), t.data_ptr() + max(t.numel() * t.element_size(), 1), name))
            self.keep.append(t)
        return t

    def name_of(self, p):
        if not p:
            return 0
        for lo, hi, name in reversed(self.spans):
            if lo <= p < hi:
                return name
        return 'tmp'

    def _arg(self, a, ctype):
        if isinstance(a, ctypes.Array):
            return [self.name_of(v) for v in a]
        if ctype is ctypes.c_void_p:
            return self.name_of(a.value if isinstance(a, ctypes.c_void_p) else a)
        return a

    def __getattr__(self, symbol):
        if symbol.endswith(HOST_SUFFIXES) or symbol in HOST_NAMES:
            return getattr(self.real, symbol)
        argtypes = _lib.SIGNATURES[symbol][1]           # (KeyError: not a symbol of the C ABI)

        def launch(*args):
            assert len(args) == len(argtypes), (symbol, len(args), len(argtypes))
            self.log.append([symbol, [self._arg(a, t) for a, t in zip(args[:-1], argtypes)]])
            return 0
        return launch

    def _split16(self, real):
        def split16(t):
            parts = [p.as_subclass(_Piece) for p in real(t)]
            base = self.name_of(t.data_ptr())
            if base not in (0, 'tmp'):
                for i, p in enumerate(parts):
                    self.name('%s.%d' % (base, i), p)
            return parts
        return split16

    def _derived(self, real, label):
        def derived(src, *args, **kwargs):
            out = real(src, *args, **kwargs)
            name = self.name_of(src.data_ptr())
            return self.name('%s(%s)' % (label, name), out) if name not in (0, 'tmp') else out
        return derived

    def install(self, monkeypatch):
        monkeypatch.setattr(_lib, 'load_library', lambda: self)
        monkeypatch.setattr(ops, 'require_cuda', lambda *tensors: None)
        monkeypatch.setattr(ops, 'stream_ptr', lambda: 0)
        monkeypatch.setattr(ops, '_workspace', lambda nbytes, device: torch.empty(max(int(nbytes), 1), dtype=torch.uint8))     # (its size is logged: exactly what was asked for)
        monkeypatch.setattr(ops, '_split16', self._split16(ops._split16))
        for fn in [n for n in dir(ops) if n.endswith('pack_weight')]:
            monkeypatch.setattr(ops, fn, self._derived(getattr(ops, fn), 'pack'))
        monkeypatch.setattr(ops, 'space_to_depth2', self._derived(ops.space_to_depth2, 'planes'))
        monkeypatch.setattr(_Piece, 'recorder', self)

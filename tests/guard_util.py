"""Guard bytes round kernel operands and outputs (a plain helper module: tests import it).

The canary is the byte 0xFF everywhere: as fp32, bf16, fp16 or fp64 it reads as NaN, as int32 as -1, so an element that was never written
poisons any comparison, and a byte outside an output's window that is no longer 0xFF was written by a kernel that had no business there.

  * `embed(t, ld, offset, ...)` copies a 2-D tensor into an all-0xFF buffer with a leading dimension and an element offset of the caller's
    choice and returns (strided view, Guard) -- a padded / misaligned INPUT whose padding is NaN.
  * `window(shape, dtype, ld, offset, device, ...)` is the same for an OUTPUT: the interior is 0xFF too.
  * `guarded_ops(monkeypatch, pad, misalign)` puts every output that the `ops` wrappers allocate (`torch.empty`, `torch.empty_like`,
    `torch.zeros` on a CUDA device) between two `pad`-byte bands of 0xFF; the band behind an output begins at the byte after its last
    element, with no rounding up.  `misalign=k` shifts the output by k elements, off 16-byte alignment.  What `ops` allocates for the
    life of the process (its workspaces and state words, PROCESS_CACHES) is left to torch: nothing of a test stays behind in those caches.

What this sees and what it does not: a stray WRITE within `pad` bytes of an output (4096 by default: more than any single vector access,
16 B, or per-wave piece, 1 KiB, of these kernels, and a multiple of 512 so that the guarded output keeps the alignment class of a plain
allocation and the kernel takes the same path).  A stray write farther out than `pad` is not caught, and neither is any out-of-range READ.
"""
import torch

from spatiotemporal_variable_separation_amd import ops

CANARY = 0xFF
ALIGN = 512            # (the alignment class of a plain caching-allocator block: the guarded middle keeps it)


class Guard:
    """One all-0xFF byte buffer and the byte ranges of it that belong to the window: rows of `row_bytes` every `ld_bytes` from `start`
    (`batch` such problems every `batch_bytes`)."""

    def __init__(self, buf, start, rows, row_bytes, ld_bytes, ordinal=0, shape=None, dtype=None, batch=1, batch_bytes=0):
        self.buf, self.start, self.rows, self.row_bytes, self.ld_bytes = buf, start, rows, row_bytes, ld_bytes
        self.batch, self.batch_bytes = batch, batch_bytes
        self.ordinal, self.shape, self.dtype = ordinal, tuple(shape) if shape is not None else None, dtype
        self._mask = None

    def _outside(self):
        if self._mask is None:
            m = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
            if self.rows and self.row_bytes:
                m.as_strided((self.batch, self.rows, self.row_bytes), (self.batch_bytes, self.ld_bytes, 1), self.start).fill_(False)
            self._mask = m
        return self._mask

    def side(self, byte):
        one = (self.rows - 1) * self.ld_bytes + self.row_bytes if self.rows else 0
        end = self.start + (self.batch - 1) * self.batch_bytes + one
        if byte < self.start:
            return 'before'
        if byte >= end:
            return 'after'
        within = (byte - self.start) % self.batch_bytes if self.batch > 1 else byte - self.start
        return 'between problems of' if within >= one else 'between rows of'

    def dirty(self):
        """Byte offsets (within the buffer) outside the window that are no longer 0xFF, ascending."""
        if self.buf.is_cuda:
            torch.cuda.synchronize(self.buf.device)
        bad = (self.buf != CANARY) & self._outside()
        return bad.nonzero().reshape(-1)

    def check(self):
        bad = self.dirty()
        if bad.numel():
            first = int(bad[0])
            raise AssertionError('allocation #%d (shape %s, %s): %d guard byte(s) overwritten, the first %s the window, at buffer byte %d '
                                 '(window byte %+d)' % (self.ordinal, self.shape, self.dtype, bad.numel(), self.side(first), first,
                                                        first - self.start))

    def assert_written(self, view):
        if view.is_cuda:
            torch.cuda.synchronize(view.device)
        v = view.double() if view.is_floating_point() else view
        holes = torch.isnan(v) if view.is_floating_point() else (v == -1)
        assert not bool(holes.any()), 'allocation #%d (shape %s, %s): %d element(s) of the window were never written (first at %s)' % (
            self.ordinal, self.shape, self.dtype, int(holes.sum()), tuple(int(i) for i in holes.nonzero()[0]))


def _carve(shape, dtype, ld, offset, rows_before, rows_after, device, batch_stride=None, ordinal=0):
    batch = shape[0] if len(shape) == 3 else 1
    rows, cols = shape[-2:]
    ld = cols if ld is None else ld
    one = (rows_before + rows + rows_after) * ld
    batch_stride = one if batch_stride is None else batch_stride
    assert ld >= cols and offset >= 0 and (batch == 1 or batch_stride >= (rows - 1) * ld + cols)
    esz = torch.empty((), dtype=dtype).element_size()
    n = offset + (batch - 1) * batch_stride + one
    buf = torch.full((n * esz,), CANARY, dtype=torch.uint8, device=device)
    first = offset + rows_before * ld
    view = buf.view(dtype).as_strided((batch, rows, cols), (batch_stride, ld, 1), first)
    guard = Guard(buf, first * esz, rows, cols * esz, ld * esz, ordinal, shape, dtype, batch, batch_stride * esz)
    return (view if len(shape) == 3 else view[0]), guard


def embed(t, ld=None, offset=0, rows_before=0, rows_after=1, batch_stride=None):
    """(view, Guard): `t` inside a fresh all-0xFF buffer, its rows `ld` elements apart and its first element `offset` elements (plus
    `rows_before` rows) past the buffer's 512-byte-aligned base.  `t` is 2-D, or -- with `batch_stride` -- 3-D (problem i starts
    `i * batch_stride` elements on); any other N-D tensor is taken as ONE row and comes back in its own shape, contiguous."""
    if batch_stride is not None:
        assert t.dim() == 3
        view, guard = _carve(tuple(t.shape), t.dtype, ld, offset, rows_before, rows_after, t.device, batch_stride)
        view.copy_(t)
        return view, guard
    t2 = t if t.dim() == 2 else t.reshape(1, -1)
    view, guard = _carve(tuple(t2.shape), t.dtype, ld, offset, rows_before, rows_after, t.device)
    view.copy_(t2)
    return (view if t.dim() == 2 else view.reshape(-1)[:t.numel()].view(t.shape)), guard


def window(shape, dtype, ld=None, offset=0, device='cpu', rows_before=0, rows_after=1, batch_stride=None):
    """(view, Guard): an output window of `shape` (2-D; 3-D with `batch_stride`), 0xFF inside and outside."""
    assert len(shape) == (3 if batch_stride is not None else 2)
    return _carve(tuple(shape), dtype, ld, offset, rows_before, rows_after, device, batch_stride)


class GuardedAllocs:
    def __init__(self, pad, misalign):
        assert pad % ALIGN == 0, 'the pad must keep the alignment class of a plain allocation'
        self.pad, self.misalign, self.guards = pad, misalign, []

    def alloc(self, shape, dtype, device, zero=False):
        shape = tuple(int(s) for s in shape)
        dtype = dtype or torch.get_default_dtype()
        esz = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        start = self.pad + self.misalign * esz
        buf = torch.full((start + numel * esz + self.pad,), CANARY, dtype=torch.uint8, device=device)
        mid = buf[start:start + numel * esz].view(dtype).view(shape)
        if zero:
            mid.zero_()
        self.guards.append(Guard(buf, start, 1, numel * esz, numel * esz, len(self.guards), shape, dtype))
        return mid

    def check(self):
        for g in self.guards:
            g.check()


class _TorchProxy:
    """`torch` for `ops`: everything is torch's own, except empty / empty_like / zeros on a CUDA device."""

    def __init__(self, allocs, guard_cpu=False):
        self._allocs, self._guard_cpu, self._paused = allocs, guard_cpu, 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def _mine(self, device):
        if device is None or self._paused:
            return False
        return torch.device(device).type == 'cuda' or self._guard_cpu

    @staticmethod
    def _shape(size):
        if len(size) == 1 and not isinstance(size[0], int):
            return tuple(size[0])
        return tuple(size)

    def _make(self, real, zero, size, kwargs):
        if not self._mine(kwargs.get('device')) or set(kwargs) - {'dtype', 'device'}:
            return real(*size, **kwargs)
        return self._allocs.alloc(self._shape(size), kwargs.get('dtype'), kwargs['device'], zero)

    def empty(self, *size, **kwargs):
        return self._make(torch.empty, False, size, kwargs)

    def zeros(self, *size, **kwargs):
        return self._make(torch.zeros, True, size, kwargs)

    def empty_like(self, t, **kwargs):
        device = kwargs.get('device', t.device)
        if not self._mine(device) or set(kwargs) - {'dtype', 'device'} or not t.is_contiguous():
            return torch.empty_like(t, **kwargs)
        return self._allocs.alloc(t.shape, kwargs.get('dtype', t.dtype), device)


# The functions of `ops` that allocate what the PROCESS keeps (grow-only workspaces per stream, the exchange guard word, the BatchNorm sum
# buffers, the one-launch layer's state): what they allocate outlives the test, so they always get torch's own, aligned allocations -- a
# guarded (let alone misaligned) carve left in one of these caches would be handed to every later call of the process.
PROCESS_CACHES = ('_workspace', '_rollout_workspace', 'exchange_guard', 'bn_sums_buffer', '_imgbn_state')


def _unguarded(proxy, fn):
    def call(*args, **kwargs):
        proxy._paused += 1
        try:
            return fn(*args, **kwargs)
        finally:
            proxy._paused -= 1
    return call


def guarded_ops(monkeypatch, pad=4096, misalign=0, guard_cpu=False):
    """From here to the end of the monkeypatch, every `torch.empty` / `empty_like` / `zeros` that `ops` makes on a CUDA device (`guard_cpu`:
    on any device, for the tests of this module itself) sits between two `pad`-byte bands of 0xFF -- except inside the PROCESS_CACHES
    functions.  Returns the GuardedAllocs: `.check()` checks every allocation made so far, `.guards` lists them in order."""
    allocs = GuardedAllocs(pad, misalign)
    proxy = _TorchProxy(allocs, guard_cpu)
    monkeypatch.setattr(ops, 'torch', proxy)
    for name in PROCESS_CACHES:
        monkeypatch.setattr(ops, name, _unguarded(proxy, getattr(ops, name)))
    return allocs

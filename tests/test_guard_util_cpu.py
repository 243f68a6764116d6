"""tests/guard_util.py on CPU tensors: the recorder stands in for the library, so nothing is launched and every 'stray write' is planted by hand."""
import pytest
import torch

from cabi_recorder import Recorder
from guard_util import CANARY, embed, guarded_ops, window
from spatiotemporal_variable_separation_amd import ops


def test_embed_gives_the_asked_strides_and_offset_and_nan_padding():
    t = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    for dtype in (torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.int32):
        v, g = embed(t.to(dtype), ld=7, offset=3, rows_before=2, rows_after=1)
        esz = v.element_size()
        assert v.stride() == (7, 1) and tuple(v.shape) == (3, 4) and torch.equal(v, t.to(dtype))
        assert v.data_ptr() - g.buf.data_ptr() == (3 + 2 * 7) * esz and g.buf.data_ptr() % 16 == 0
        assert g.buf.numel() == (3 + 6 * 7) * esz
        whole = g.buf.view(dtype)
        if dtype is torch.int32:
            assert int((whole == -1).sum()) == whole.numel() - 12
        else:
            assert int(torch.isnan(whole.double()).sum()) == whole.numel() - 12
        g.check()
        g.assert_written(v)
    flat, g = embed(torch.arange(24.).reshape(2, 3, 4), offset=1)
    assert tuple(flat.shape) == (2, 3, 4) and flat.is_contiguous() and flat.data_ptr() - g.buf.data_ptr() == 4
    assert torch.equal(flat, torch.arange(24.).reshape(2, 3, 4))


def test_window_is_poisoned_inside_and_assert_written_sees_a_hole():
    v, g = window((3, 5), torch.bfloat16, ld=9, offset=1)
    assert v.stride() == (9, 1) and bool(torch.isnan(v.float()).all())
    g.check()
    with pytest.raises(AssertionError, match='never written'):
        g.assert_written(v)
    v.fill_(1.0)
    g.assert_written(v)
    g.check()
    v[2, 4] = float('nan')
    with pytest.raises(AssertionError, match=r'1 element\(s\) of the window were never written \(first at \(2, 4\)\)'):
        g.assert_written(v)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_one_flipped_byte_is_reported_with_its_side_and_offset(dtype):
    esz = torch.empty((), dtype=dtype).element_size()
    rows, cols, ld, off = 3, 5, 8, 2

    def fresh():
        v, g = window((rows, cols), dtype, ld=ld, offset=off, rows_before=1, rows_after=1)
        v.fill_(0.5)
        return g

    start = (off + ld) * esz
    end = start + (2 * ld + cols) * esz
    last = (off + 5 * ld) * esz - 1
    for byte, side in ((start - 1, 'before'), (0, 'before'), (end, 'after'), (last, 'after'),
                       (start + cols * esz, 'between rows of'), (start + ld * esz - 1, 'between rows of'), (start + (ld + cols) * esz, 'between rows of')):
        g = fresh()
        g.check()
        g.buf[byte] = 0x7F
        with pytest.raises(AssertionError) as e:
            g.check()
        msg = str(e.value)
        assert 'allocation #0 (shape (3, 5), %s)' % dtype in msg and 'the first %s the window, at buffer byte %d ' % (side, byte) in msg, msg
        assert '1 guard byte(s)' in msg
    g = fresh()                                 # every byte INSIDE the window may change
    for r in range(rows):
        g.buf[start + r * ld * esz:start + (r * ld + cols) * esz] = 0
    g.check()


def test_a_batched_window_guards_the_bytes_between_its_problems():
    rows, cols, ld, bs = 2, 3, 4, 11
    v, g = window((3, rows, cols), torch.float32, ld=ld, offset=1, batch_stride=bs, rows_after=0)
    assert v.stride() == (bs, ld, 1) and g.buf.numel() == (1 + 2 * bs + rows * ld) * 4
    v.fill_(1.0)
    g.check()
    one = ((rows - 1) * ld + cols) * 4
    for byte, side in ((3, 'before'), (4 + cols * 4, 'between rows of'), (4 + one, 'between problems of'), (4 + bs * 4 - 1, 'between problems of'),
                       (4 + bs * 4 + cols * 4, 'between rows of'), (4 + 2 * bs * 4 + one, 'after')):
        g.buf[byte] = 1
        with pytest.raises(AssertionError, match='the first %s the window, at buffer byte %d ' % (side, byte)):
            g.check()
        g.buf[byte] = CANARY
    g.check()
    t = torch.arange(12.).reshape(2, 2, 3)
    e, g = embed(t, ld=5, offset=2, batch_stride=13)
    assert torch.equal(e, t) and e.stride() == (13, 5, 1) and e.data_ptr() - g.buf.data_ptr() == 8
    g.check()


def _cpu_ops(monkeypatch, **kw):
    rec = Recorder()
    rec.install(monkeypatch)
    return rec, guarded_ops(monkeypatch, guard_cpu=True, **kw)


def test_the_proxy_covers_empty_empty_like_and_zeros(monkeypatch):
    _, allocs = _cpu_ops(monkeypatch)
    proxy = ops.torch
    assert proxy is not torch and proxy.float32 is torch.float32 and proxy.Tensor is torch.Tensor and proxy.cuda is torch.cuda
    a = proxy.empty((3, 5), dtype=torch.float32, device='cpu')
    b = proxy.empty(3, 5, dtype=torch.bfloat16, device='cpu')
    c = proxy.empty(torch.Size((2, 3, 5)), dtype=torch.float16, device=torch.device('cpu'))
    d = proxy.empty_like(a)
    e = proxy.empty_like(a, dtype=torch.float64)
    z = proxy.zeros((7,), dtype=torch.float32, device='cpu')
    z2 = proxy.zeros(2, 3, dtype=torch.int32, device='cpu')
    s = proxy.empty((), dtype=torch.float32, device='cpu')
    got = [a, b, c, d, e, z, z2, s]
    assert [tuple(t.shape) for t in got] == [(3, 5), (3, 5), (2, 3, 5), (3, 5), (3, 5), (7,), (2, 3), ()]
    assert [t.dtype for t in got] == [torch.float32, torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.float32, torch.int32, torch.float32]
    assert len(allocs.guards) == 8 and [g.ordinal for g in allocs.guards] == list(range(8))
    for t, g in zip(got, allocs.guards):
        nbytes = t.numel() * t.element_size()
        assert t.is_contiguous() and g.buf.numel() == 4096 + nbytes + 4096          # (no rounding up: the guard begins at the next byte)
        assert t.data_ptr() - g.buf.data_ptr() == 4096 and g.start == 4096 and g.row_bytes == nbytes
    for t in (a, b, c, d, e):
        assert bool(torch.isnan(t.double()).all())
    assert bool((z == 0).all()) and bool((z2 == 0).all())
    assert bool((allocs.guards[5].buf[:4096] == CANARY).all()) and bool((allocs.guards[5].buf[4096 + 28:] == CANARY).all())
    allocs.check()
    # no device (a host scalar) or an argument the proxy does not know: torch's own
    assert not torch.isnan(proxy.zeros(3)).any() and len(allocs.guards) == 8
    proxy.empty((2,), dtype=torch.float32, device='cpu', pin_memory=False)
    assert len(allocs.guards) == 8


def test_misalign_shifts_every_allocation_by_whole_elements(monkeypatch):
    _, allocs = _cpu_ops(monkeypatch, misalign=1)
    for dtype, esz in ((torch.float32, 4), (torch.bfloat16, 2), (torch.float64, 8)):
        t = ops.torch.empty((5, 3), dtype=dtype, device='cpu')
        g = allocs.guards[-1]
        assert t.data_ptr() - g.buf.data_ptr() == 4096 + esz and t.data_ptr() % 16 == esz
        assert g.buf.numel() == 4096 + esz + 15 * esz + 4096
    allocs.check()


def test_the_wrappers_run_through_the_proxy_and_a_planted_byte_names_its_allocation(monkeypatch):
    rec, allocs = _cpu_ops(monkeypatch)
    x = torch.randn(4, 3, 5, 5)
    mean, invstd = ops.bn_stats(x, torch.zeros(3), torch.ones(3))
    assert len(allocs.guards) == 3 and [g.shape for g in allocs.guards] == [(1, 3)] * 3
    y = ops.bn_act_fwd(x, mean, invstd, torch.ones(3), torch.zeros(3), 'relu', torch.bfloat16)
    assert allocs.guards[3].shape == (4, 3, 5, 5) and allocs.guards[3].dtype is torch.bfloat16
    a, b = torch.randn(6, 8), torch.randn(5, 8)
    out = ops.gemm(a, 0, b, 0, 6, 5, 8)
    assert [name for name, _ in rec.log] == ['vs_bn_stats', 'vs_bn_act_fwd', 'vs_gemm']
    g_out = allocs.guards[-1]
    assert g_out.shape == (6, 5) and out.data_ptr() == g_out.buf.data_ptr() + 4096
    allocs.check()

    cases = ((3, 4096 - 1, 'before', -1), (3, 4096 + y.numel() * 2, 'after', y.numel() * 2),
             (len(allocs.guards) - 1, g_out.buf.numel() - 1, 'after', 120 + 4095), (0, 0, 'before', -4096))
    for ordinal, byte, side, rel in cases:
        g = allocs.guards[ordinal]
        g.buf[byte] = 0
        with pytest.raises(AssertionError) as e:
            allocs.check()
        msg = str(e.value)
        assert msg.startswith('allocation #%d (shape %s, %s)' % (ordinal, g.shape, g.dtype)), msg
        assert 'the first %s the window, at buffer byte %d (window byte %+d)' % (side, byte, rel) in msg, msg
        g.buf[byte] = CANARY
        allocs.check()


def test_undoing_the_monkeypatch_gives_ops_its_torch_back():
    mp = pytest.MonkeyPatch()
    guarded_ops(mp)
    assert ops.torch is not torch
    mp.undo()
    assert ops.torch is torch


def test_cpu_allocations_are_left_alone_by_default(monkeypatch):
    allocs = guarded_ops(monkeypatch)
    t = ops.torch.empty((4,), dtype=torch.float32, device='cpu')
    z = ops.torch.zeros((4,), dtype=torch.float32, device=torch.device('cpu'))
    assert not allocs.guards and tuple(t.shape) == (4,) and bool((z == 0).all())


def test_a_guarded_call_leaves_nothing_of_its_own_in_the_process_caches(monkeypatch):
    """ops._workspace keeps one grow-only buffer per (device, stream) for the life of the process.  The REAL function runs here (the stream
    lookup answered for a CPU device): a guarded, misaligned call that is the first to need the buffer caches one of torch's own
    allocations, never a carve of a guard buffer, and a call that finds the buffer filled leaves the cache as it was."""
    import types
    from guard_util import PROCESS_CACHES
    real_workspace = ops._workspace
    rec = Recorder()
    rec.install(monkeypatch)
    monkeypatch.setattr(ops, '_workspace', real_workspace)              # (the recorder's stand-in does not cache)
    monkeypatch.setattr(ops, '_ws_cache', {})
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda device=None: types.SimpleNamespace(cuda_stream=0))
    allocs = guarded_ops(monkeypatch, misalign=1, guard_cpu=True)
    assert all(getattr(ops, name).__name__ == 'call' for name in PROCESS_CACHES)
    x = torch.randn(3, 5, 8, 8).bfloat16()
    out = ops.chan_sum(x)
    M, N, K = 100, 70, 4104                                             # a split-K problem: vs_gemm takes slabs from the workspace
    assert rec.real.vs_gemm_workspace_bytes(M, N, K) > 0
    c = ops.gemm(torch.randn(M, K), 0, torch.randn(N, K), 0, M, N, K)
    assert [name for name, _ in rec.log] == ['vs_chan_sum_ws', 'vs_gemm']
    assert len(allocs.guards) == 2 and out.data_ptr() % 16 == 4 and c.data_ptr() % 16 == 4         # the outputs ARE guarded and off alignment
    assert len(ops._ws_cache) == 1
    (ws,) = ops._ws_cache.values()
    assert ws.data_ptr() % 16 == 0 and ws.dtype == torch.uint8
    for g in allocs.guards:
        assert not (g.buf.data_ptr() <= ws.data_ptr() < g.buf.data_ptr() + g.buf.numel()), 'the cached workspace is a carve of guard allocation #%d' % g.ordinal
    before = dict(ops._ws_cache)
    ops.chan_sum(x)
    ops.gemm(torch.randn(M, K), 0, torch.randn(N, K), 0, M, N, K)
    assert ops._ws_cache.keys() == before.keys() and all(ops._ws_cache[k] is before[k] for k in before)
    allocs.check()

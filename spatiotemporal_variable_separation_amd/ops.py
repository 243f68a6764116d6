"""Thin tensor-level wrappers over the C ABI (include/varsep_hip.h).  No autograd here; see functional.py."""
import collections
import os

import torch

from . import _lib
from ._lib import F32, BF16, F16, ACT, LAYOUT_R, LAYOUT_S, check, code_of, dtype_code, stream_ptr, require_cuda

_DT = {F32: 'f32', BF16: 'bf16', F16: 'fp16'}

_ws_cache = {}
_retired = []

# ---- optional per-launch timing with HIP events on the launch stream (bench.py: roofline of the dominant kernel) ----
_PROF = {'on': False, 'events': []}
_LNAME = {0: 'R', 1: 'S'}


def profile_reset(enable=True, pool=0):
    """Start (or stop) per-launch event timing.  `pool` events are created and recorded once up front so that the timed
    region only re-records existing HIP events (creating thousands of events inside the region slows the host)."""
    _PROF['on'] = enable
    _PROF['events'] = []
    _PROF['pool'] = []
    if enable and pool:
        for _ in range(pool):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            _PROF['pool'].append(e)
        torch.cuda.synchronize()


def _new_event():
    pool = _PROF.get('pool')
    e = pool.pop() if pool else torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _pb():
    if not _PROF['on']:
        return None
    return _new_event()


def _pe(e0, name, flops=0.0, nbytes=0.0):
    if e0 is None:
        return
    _PROF['events'].append((name, e0, _new_event(), flops, nbytes))


def profile_collect():
    """{kernel family: {'ms': summed event time, 'n': launches, 'flops': algorithmic FLOPs, 'bytes': algorithmic bytes}}"""
    torch.cuda.synchronize()
    out = {}
    for name, e0, e1, fl, by in _PROF['events']:
        r = out.setdefault(name, {'ms': 0.0, 'n': 0, 'flops': 0.0, 'bytes': 0.0})
        r['ms'] += e0.elapsed_time(e1)
        r['n'] += 1
        r['flops'] += fl
        r['bytes'] += by
    _PROF['on'] = False
    _PROF['events'] = []
    return out


def _workspace(nbytes, device):
    """One grow-only split-K workspace per (device, stream): launches on different streams may overlap, and a workspace is only
    ordered by the stream it is used on (allocated by torch, so legal inside graph capture after warm-up)."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _retired.append(buf)      # a recorded hipGraph may hold its address: outgrown workspaces are never freed
        buf = torch.empty(max(nbytes, 2 * buf.numel() if buf is not None else 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def gemm(a, layout_a, b, layout_b, M, N, K, out=None, out_dtype=torch.float32, alpha=1.0, bias=None, act='none',
         mask=None, mask_act='none', accumulate=False, lda=None, ldb=None):
    """out[M,N] = epi(sum_k A(m,k) B(n,k)); A/B are 2-D (possibly row-strided) tensors of identical dtype."""
    require_cuda(a, b, out, bias, mask)
    lib = _lib.load_library()
    if a.dtype != b.dtype:
        raise _lib.VarsepHipError('gemm operands must share a dtype (%s vs %s)' % (a.dtype, b.dtype))
    assert a.stride(-1) == 1 and b.stride(-1) == 1
    compute = dtype_code(a)
    lda = a.stride(0) if lda is None else lda
    ldb = b.stride(0) if ldb is None else ldb
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=a.device)
    assert out.stride(-1) == 1
    ws_bytes = lib.vs_gemm_workspace_bytes(M, N, K)
    ws = _workspace(ws_bytes, a.device) if ws_bytes else None
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.is_contiguous()
    e0 = _pb()
    check(lib.vs_gemm(compute, M, N, K, a.data_ptr(), lda, layout_a, b.data_ptr(), ldb, layout_b, out.data_ptr(),
                      out.stride(0), dtype_code(out), float(alpha), _ptr(bias), ACT[act], _ptr(mask),
                      mask.stride(0) if mask is not None else 0, dtype_code(mask) if mask is not None else 0,
                      ACT[mask_act], int(bool(accumulate)), _ptr(ws), ws.numel() if ws is not None else 0, stream_ptr()),
          'vs_gemm')
    _pe(e0, 'vs_gemm<%s,%s%s>' % (_DT[compute], _LNAME[layout_a], _LNAME[layout_b]),
        flops=2.0 * M * N * K, nbytes=float((M * K + N * K) * a.element_size() + M * N * out.element_size()))
    return out


def gemm_adam(a, layout_a, b, layout_b, M, N, K, param, exp_avg, exp_avg_sq, shadow, step_dev, skipped, lr, betas, eps, alpha=1.0):
    """param [M, N] (fp32, contiguous) takes one Adam step with G = alpha * A B^T as its gradient; G is never stored
    (vs_gemm_adam).  Raises VarsepHipError(code VS_ERR_UNSUPPORTED) when the operands do not fit the LDS-DMA loader."""
    require_cuda(a, b, param, exp_avg, exp_avg_sq, step_dev)
    lib = _lib.load_library()
    assert a.dtype == b.dtype and a.dtype in (torch.bfloat16, torch.float16) and a.stride(-1) == 1 and b.stride(-1) == 1
    assert param.dtype == torch.float32 and param.is_contiguous() and tuple(param.shape) == (M, N)
    assert exp_avg.is_contiguous() and exp_avg_sq.is_contiguous() and exp_avg.shape == param.shape == exp_avg_sq.shape
    assert shadow is None or (shadow.is_contiguous() and shadow.shape == param.shape and shadow.dtype in (torch.bfloat16, torch.float16))
    e0 = _pb()
    check(lib.vs_gemm_adam(dtype_code(a), M, N, K, a.data_ptr(), a.stride(0), layout_a, b.data_ptr(), b.stride(0), layout_b, float(alpha),
                           param.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), _ptr(shadow),
                           code_of(shadow.dtype) if shadow is not None else BF16, step_dev.data_ptr(), int(skipped), float(lr),
                           float(betas[0]), float(betas[1]), float(eps), stream_ptr()), 'vs_gemm_adam')
    # algorithmic bytes: the operands, p / m / v read and written, the 16-bit copy
    _pe(e0, 'vs_gemm_adam<%s,%s%s>' % (_DT[dtype_code(a)], _LNAME[layout_a], _LNAME[layout_b]), flops=2.0 * M * N * K,
        nbytes=float((M * K + N * K) * a.element_size() + M * N * (24 + (2 if shadow is not None else 0))))


_PACED = {'launches': 0}


def gemm_adam_paced_launches():
    """How many paced fused updates (gemm_adam_paced) this process has issued or recorded."""
    return _PACED['launches']


def gemm_adam_paced(a, layout_a, b, layout_b, M, N, K, param, exp_avg, exp_avg_sq, shadow, step_dev, skipped, lr, betas, eps,
                    max_workgroups, pieces_in_flight, cache_policy, alpha=1.0):
    """gemm_adam as a launch of at most `max_workgroups` workgroups that walk the tiles (vs_gemm_adam_paced): bit for bit the same
    update, for running beside a latency-bound kernel.  param, moments and the 16-bit copy may be row-strided views with ONE leading
    dimension (param.stride(0))."""
    require_cuda(a, b, param, exp_avg, exp_avg_sq, step_dev)
    lib = _lib.load_library()
    assert a.dtype == b.dtype and a.dtype in (torch.bfloat16, torch.float16) and a.stride(-1) == 1 and b.stride(-1) == 1
    assert param.dtype == torch.float32 and tuple(param.shape) == (M, N)
    ldp = param.stride(0)
    for t in (param, exp_avg, exp_avg_sq, shadow):
        assert t is None or (t.shape == param.shape and t.stride(1) == 1 and t.stride(0) == ldp)
    assert shadow is None or shadow.dtype in (torch.bfloat16, torch.float16)
    e0 = _pb()
    check(lib.vs_gemm_adam_paced(dtype_code(a), M, N, K, a.data_ptr(), a.stride(0), layout_a, b.data_ptr(), b.stride(0), layout_b, float(alpha),
                                 param.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), _ptr(shadow), ldp,
                                 code_of(shadow.dtype) if shadow is not None else BF16, step_dev.data_ptr(), int(skipped), float(lr),
                                 float(betas[0]), float(betas[1]), float(eps), int(max_workgroups), int(pieces_in_flight), int(cache_policy),
                                 stream_ptr()), 'vs_gemm_adam_paced')
    _PACED['launches'] += 1
    _pe(e0, 'vs_gemm_adam<%s,%s%s>paced' % (_DT[dtype_code(a)], _LNAME[layout_a], _LNAME[layout_b]), flops=2.0 * M * N * K,
        nbytes=float((M * K + N * K) * a.element_size() + M * N * (24 + (2 if shadow is not None else 0))))


def gemm_batched(a, layout_a, b, layout_b, M, N, K, out_dtype=torch.float32, out=None):
    """a [batch, ., .], b [batch, ., .] contiguous 3-D tensors of one dtype: out[i] = A_i B_i^T for every i in ONE launch."""
    require_cuda(a, b)
    lib = _lib.load_library()
    if a.dtype != b.dtype:
        raise _lib.VarsepHipError('gemm operands must share a dtype (%s vs %s)' % (a.dtype, b.dtype))
    assert a.dim() == 3 and b.dim() == 3 and a.is_contiguous() and b.is_contiguous() and a.shape[0] == b.shape[0]
    batch = a.shape[0]
    compute = dtype_code(a)
    if out is None:
        out = torch.empty((batch, M, N), dtype=out_dtype, device=a.device)
    assert out.is_contiguous() and tuple(out.shape) == (batch, M, N)
    ws_bytes = lib.vs_gemm_batched_workspace_bytes(batch, M, N, K)
    ws = _workspace(ws_bytes, a.device) if ws_bytes else None
    e0 = _pb()
    check(lib.vs_gemm_batched(compute, batch, M, N, K, a.data_ptr(), a.stride(1), a.stride(0), layout_a, b.data_ptr(), b.stride(1),
                              b.stride(0), layout_b, out.data_ptr(), N, M * N, dtype_code(out), 1.0, 0, _ptr(ws),
                              ws.numel() if ws is not None else 0, stream_ptr()), 'vs_gemm_batched')
    _pe(e0, 'vs_gemm<%s,%s%s>' % (_DT[compute], _LNAME[layout_a], _LNAME[layout_b]),
        flops=2.0 * batch * M * N * K, nbytes=float(batch * ((M * K + N * K) * a.element_size() + M * N * out.element_size())))
    return out


def cast(src, dtype, out=None):
    require_cuda(src)
    src = src.contiguous()
    if out is None:
        out = torch.empty(src.shape, dtype=dtype, device=src.device)
    check(_lib.load_library().vs_cast(src.data_ptr(), dtype_code(src), out.data_ptr(), dtype_code(out), src.numel(),
                                      stream_ptr()), 'vs_cast')
    return out


def copy2d(src, rows, cols, lds, out, ldd, col_offset_dev=None, col_offset_scale=0, src_elem_offset=0):
    require_cuda(src, out)
    esz = src.element_size()
    check(_lib.load_library().vs_copy2d(src.data_ptr() + src_elem_offset * esz, dtype_code(src), lds, out.data_ptr(),
                                        dtype_code(out), ldd, rows, cols, _ptr(col_offset_dev), col_offset_scale,
                                        stream_ptr()), 'vs_copy2d')
    return out


def copy2d_pair(src, rows, cols, lds, out, ldd, col_offset_dev, col_offset_scale, elem_offset_a, elem_offset_b):
    """out[0:rows] = window of `src` rows at elem_offset_a + *col_offset_dev * col_offset_scale, out[rows:2 rows] = the window at
    elem_offset_b, one launch (with the element-type conversion)."""
    require_cuda(src, out)
    check(_lib.load_library().vs_copy2d_pair(src.data_ptr(), dtype_code(src), lds, out.data_ptr(), dtype_code(out), ldd, rows, cols,
                                             _ptr(col_offset_dev), col_offset_scale, elem_offset_a, elem_offset_b, stream_ptr()), 'vs_copy2d_pair')
    return out


def colsum(x, M, N, out=None, accumulate=False):
    require_cuda(x)
    if out is None:
        out = torch.empty((N,), dtype=torch.float32, device=x.device)
    check(_lib.load_library().vs_colsum(x.data_ptr(), dtype_code(x), x.stride(0), M, N, out.data_ptr(),
                                        int(bool(accumulate)), stream_ptr()), 'vs_colsum')
    return out


def colsum_alloc(jobs, flat=None):
    """(flat, views): the result vectors colsum_multi(jobs) would allocate, for callers that launch it later (zero_flat=flat)."""
    if flat is None:
        flat = torch.empty((sum(x.shape[1] for x in jobs),), dtype=torch.float32, device=jobs[0].device)
    views, off = [], 0
    for x in jobs:
        views.append(flat[off:off + x.shape[1]])
        off += x.shape[1]
    return flat, views


def colsum_multi(jobs, outs=None, zero_flat=None):
    """jobs: list of (x [M, N] 2-D tensor).  Returns one fp32 vector of column sums per job (views of one flat buffer),
    computed by a single launch (+ one memset).  `outs`: caller-provided fp32 vectors that are ALREADY ZERO (the partial sums
    are added to them, e.g. slices of a zeroed all-reduce bucket) -- then nothing is allocated or filled here; with `zero_flat`
    (colsum_alloc) they are consecutive views of that buffer and are zeroed by the launch."""
    import ctypes
    results = []
    for i in range(0, len(jobs), 12):
        chunk = jobs[i:i + 12]
        n = len(chunk)
        require_cuda(*chunk)
        total = sum(x.shape[1] for x in chunk)
        if outs is None:
            flat = torch.empty((total,), dtype=torch.float32, device=chunk[0].device)
            views, off = [], 0
            for x in chunk:
                views.append(flat[off:off + x.shape[1]])
                off += x.shape[1]
            zero_base, zero_count = flat.data_ptr(), total
        else:
            views = outs[i:i + 12]
            for v, x in zip(views, chunk):
                assert v.dtype == torch.float32 and v.is_contiguous() and v.numel() == x.shape[1]
            require_cuda(*views)
            zero_base, zero_count = None, 0
            if zero_flat is not None:
                zero_base, zero_count = views[0].data_ptr(), sum(v.numel() for v in views)
        VP, I32, I64 = ctypes.c_void_p * n, ctypes.c_int * n, ctypes.c_int64 * n
        e0 = _pb()
        check(_lib.load_library().vs_colsum_multi(
            n, VP(*[x.data_ptr() for x in chunk]), I32(*[dtype_code(x) for x in chunk]), I64(*[x.stride(0) for x in chunk]),
            I64(*[x.shape[0] for x in chunk]), I64(*[x.shape[1] for x in chunk]), VP(*[v.data_ptr() for v in views]),
            zero_base, zero_count, stream_ptr()), 'vs_colsum_multi')
        _pe(e0, 'vs_colsum_multi', nbytes=float(sum(x.numel() * x.element_size() for x in chunk)))
        results += list(views)
    return results


def act_fwd(x, act, out=None, out_dtype=None):
    require_cuda(x)
    x = x.contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype or x.dtype, device=x.device)
    check(_lib.load_library().vs_act_fwd(x.data_ptr(), dtype_code(x), out.data_ptr(), dtype_code(out), ACT[act],
                                         x.numel(), stream_ptr()), 'vs_act_fwd')
    return out


def act_bwd(dy, y, act, out_dtype=None):
    require_cuda(dy, y)
    dy, y = dy.contiguous(), y.contiguous()
    out = torch.empty(dy.shape, dtype=out_dtype or dy.dtype, device=dy.device)
    check(_lib.load_library().vs_act_bwd(dy.data_ptr(), dtype_code(dy), y.data_ptr(), dtype_code(y), out.data_ptr(),
                                         dtype_code(out), ACT[act], dy.numel(), stream_ptr()), 'vs_act_bwd')
    return out


def transpose_cast(src, dtype, out=None):
    """out[c, r] = src[r, c] converted to `dtype` (2-D, contiguous)."""
    require_cuda(src)
    assert src.dim() == 2 and src.is_contiguous()
    rows, cols = src.shape
    if out is None:
        out = torch.empty((cols, rows), dtype=dtype, device=src.device)
    check(_lib.load_library().vs_transpose_cast(src.data_ptr(), dtype_code(src), out.data_ptr(), dtype_code(out), rows,
                                                cols, stream_ptr()), 'vs_transpose_cast')
    return out


_roll_ws = {}


def _rollout_workspace(nbytes, device, geometry):
    """Exchange area of the multi-workgroup rollout: one per device AND geometry (compute type, B, C, H), zero-filled here once and then left to
    the library -- the weight-stationary form keeps per-slab epoch words in it and never clears it (include/varsep_hip.h), so an area is
    never shared between layouts."""
    if not nbytes:
        return None
    key = (device.index,) + tuple(geometry)
    buf = _roll_ws.get(key)
    if buf is None or buf.numel() != nbytes:
        buf = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        _roll_ws[key] = buf
    return buf


_GUARD = {}


def exchange_guard(device):
    """The process's exchange guard word (include/varsep_hip.h: vs_exchange_guard_set): one int32 device word that the kernels with a bounded
    in-launch exchange raise on a time-out and that every optimizer launch reads first (non-zero: no update).  Created and registered at the
    first use of such a kernel -- forward, i.e. before the step's first optimizer launch is issued or recorded.  One GPU per process (8e):
    a second device in the same process keeps the per-workspace words."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    if index in _GUARD:
        return _GUARD[index]
    lib = _lib.load_library()
    if _GUARD or lib.vs_exchange_guard_get():
        _GUARD[index] = None
        return None
    word = torch.zeros((4,), dtype=torch.int32, device=device)              # (16 bytes: a line of its own would be better still; it is read-mostly)
    check(lib.vs_exchange_guard_set(word.data_ptr()), 'vs_exchange_guard_set')
    check(lib.vs_exchange_skip_counter_set(word.data_ptr() + 4), 'vs_exchange_skip_counter_set')      # word[1]: steps the guard made the optimizer skip
    _GUARD[index] = word
    return word


def exchange_skipped_steps(device, reset=True):
    """How many optimisation steps the raised guard word has made the step-count kernel skip since the last call (0 without a guard).
    Synchronises the device (reads a word)."""
    device = torch.device(device) if not isinstance(device, torch.device) else device
    index = device.index if device.index is not None else torch.cuda.current_device()
    guard = _GUARD.get(index)
    if guard is None:
        return 0
    n = int(guard[1].item())
    if reset and n:
        guard[1].zero_()
    return n


def rollout_exchange_error(device, reset=True):
    """Non-zero iff a bounded spin of an in-launch exchange timed out in any launch since the last call (the words are sticky: the
    library never clears them): bit 1 = the MLP integrator, bit 2 = the one-launch ConvResBlock layers.  Synchronises the device (reads words)."""
    device = torch.device(device) if not isinstance(device, torch.device) else device
    index = device.index if device.index is not None else torch.cuda.current_device()
    err = 0
    guard = _GUARD.get(index)
    if guard is not None:
        err |= int(guard[0].item())
        if reset and err:
            guard[0].zero_()
    for key, buf in list(_roll_ws.items()):
        if key[0] != index:
            continue
        word = buf[buf.numel() // 16 * 16 - 16:buf.numel() // 16 * 16 - 12].view(torch.int32)
        e1 = int(word.item())
        err |= e1
        if reset and e1:
            word.zero_()
    st = _IMGBN.get(index)                              # the fused ConvResBlock layers' exchange (conv3_img16_bn_*): word 1 of their workspace
    if st is not None:
        e2 = int(st['ws'][1].item())
        if e2:
            err |= 2
            if reset:
                st['ws'][1].zero_()
    return err


_XL_PROBED = set()


def rollout_xcd_local(allowed=None):
    """Process-wide switch of the integrator's XCD-local exchange (None: leave).  False selects the placement-independent agent-scope stores."""
    if allowed is not None:
        check(_lib.load_library().vs_mlp_rollout_xcd_local_set(1 if allowed else 0), 'vs_mlp_rollout_xcd_local_set')


def _probe_rollout_exchange(code, B, C, H, nb, device):
    """START-UP decision of the exchange mode (once per device and geometry, outside stream captures).  The XCD-local form of the
    weight-stationary integrator (csrc/vs_rollout.hip, wsr::gstore<true>) leans on workgroups 8 apart sharing an XCD, which HIP does not
    promise.  One probe rollout -- three steps on zero weights, a fresh zero-filled exchange area, a short spin limit -- either completes (the
    property holds on this device / runtime: keep the 210 ns hops) or leaves the error word raised: then every launch of this process uses
    the agent-scope stores (385 ns hops, any placement).  A mid-run change of the dispatch order is still caught by the epoch tags -> the
    guard word -> skipped optimizer steps -> train.recover_exchange."""
    import sys
    key = (device.index, code, B, C, H, nb)
    if key in _XL_PROBED or torch.cuda.is_current_stream_capturing():
        return
    _XL_PROBED.add(key)
    lib = _lib.load_library()
    if not lib.vs_mlp_rollout_xcd_local_get(code, B, C, H, nb) or os.environ.get('VARSEP_ROLLOUT_PROBE', '1') == '0':
        return
    import ctypes
    dt = {BF16: torch.bfloat16, F16: torch.float16}[code]
    nbytes = lib.vs_mlp_rollout_workspace_bytes(code, B, C, H)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    n = 3
    weights = []
    for _ in range(nb):
        for (N, K) in ((H, C), (H, H), (C, H)):
            weights.append(torch.zeros((lib.vs_rollout_packed_elems(code, N, K),), dtype=dt, device=device))
    biases = []
    for _ in range(nb):
        biases += [torch.zeros((H,), device=device), torch.zeros((H,), device=device), torch.zeros((C,), device=device)]
    x0 = torch.zeros((B, C), device=device)
    t_codes = torch.empty((B, n, C), device=device)
    xin = torch.empty((nb, n - 1, B, C), dtype=dt, device=device)
    h1 = torch.empty((nb, n - 1, B, H), dtype=dt, device=device)
    h2 = torch.empty((nb, n - 1, B, H), dtype=dt, device=device)
    parts = lib.vs_mlp_rollout_parts(code, B, C, H)
    Bp = (B + 15) // 16 * 16
    m1 = torch.empty((nb, n - 1, Bp, parts, 32), dtype=torch.int32, device=device)
    m2 = torch.empty_like(m1)
    guard = _GUARD.get(device.index if device.index is not None else torch.cuda.current_device())
    before = int(guard[0].item()) if guard is not None else 0
    saved = os.environ.get('VS_ROLLOUT_SPIN_LIMIT')
    os.environ['VS_ROLLOUT_SPIN_LIMIT'] = str(1 << 16)
    try:
        wa, ba = _ptr_array(weights), _ptr_array(biases)
        check(lib.vs_mlp_rollout_fwd(code, B, C, H, nb, n, x0.data_ptr(), ctypes.cast(wa, ctypes.c_void_p), ctypes.cast(ba, ctypes.c_void_p),
                                     t_codes.data_ptr(), None, xin.data_ptr(), h1.data_ptr(), h2.data_ptr(), m1.data_ptr(), m2.data_ptr(),
                                     ws.data_ptr(), ws.numel(), stream_ptr()), 'vs_mlp_rollout_fwd (placement probe)')
        torch.cuda.current_stream().synchronize()
    finally:
        if saved is None:
            os.environ.pop('VS_ROLLOUT_SPIN_LIMIT', None)
        else:
            os.environ['VS_ROLLOUT_SPIN_LIMIT'] = saved
    if guard is not None:
        failed = int(guard[0].item()) != 0
        guard[0].fill_(before)                               # the probe's verdict is consumed here; an earlier error stays
    else:
        failed = int(ws[ws.numel() // 16 * 16 - 16:ws.numel() // 16 * 16 - 12].view(torch.int32).item()) != 0
    if failed:
        rollout_xcd_local(False)
        sys.stderr.write('varsep: the integrator\'s XCD-local exchange did not complete its start-up probe on this device (workgroups 8 apart do not '
                         'share an XCD here): using the agent-scope exchange for this process\n')


def _ptr_array(tensors):
    import ctypes
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr


def pack_rollout_weight(w, dtype, transpose, out=None):
    """fp32 master weight [rows, cols] -> packed MFMA-fragment order in `dtype` (logical L = w or w^T)."""
    require_cuda(w)
    assert w.dim() == 2 and w.is_contiguous() and w.dtype == torch.float32
    N, K = (w.shape[1], w.shape[0]) if transpose else (w.shape[0], w.shape[1])
    lib = _lib.load_library()
    code = code_of(dtype)
    n = lib.vs_rollout_packed_elems(code, N, K)
    if out is None:
        out = torch.empty((n,), dtype=dtype, device=w.device)
    check(lib.vs_pack_rollout_weight(code, w.data_ptr(), int(bool(transpose)), N, K, out.data_ptr(), stream_ptr()),
          'vs_pack_rollout_weight')
    return out


def pack_rollout_weights(jobs, dtype):
    """jobs: list of (fp32 weight [rows, cols], transpose, out buffer or None).  One launch; returns the packed buffers."""
    import ctypes
    lib = _lib.load_library()
    code = code_of(dtype)
    outs = []
    for i in range(0, len(jobs), 48):
        chunk = jobs[i:i + 48]
        n = len(chunk)
        Ns, Ks, bufs = [], [], []
        for w, tr, out in chunk:
            require_cuda(w)
            assert w.dim() == 2 and w.is_contiguous() and w.dtype == torch.float32
            N, K = (w.shape[1], w.shape[0]) if tr else (w.shape[0], w.shape[1])
            if out is None:
                out = torch.empty((lib.vs_rollout_packed_elems(code, N, K),), dtype=dtype, device=w.device)
            Ns.append(N); Ks.append(K); bufs.append(out)
        VP, I32 = ctypes.c_void_p * n, ctypes.c_int * n
        check(lib.vs_pack_rollout_weights(code, n, VP(*[w.data_ptr() for w, _, _ in chunk]), I32(*[int(bool(tr)) for _, tr, _ in chunk]),
                                          I32(*Ns), I32(*Ks), VP(*[b.data_ptr() for b in bufs]), stream_ptr()), 'vs_pack_rollout_weights')
        outs += bufs
    return outs


def mlp_rollout_fwd(x0, weights, biases, n_steps, H, want_residuals=True):
    """weights: packed [W1,W2,W3]*n_blocks in the compute dtype; biases fp32.  Returns (t_codes, residuals, saves)."""
    import ctypes
    require_cuda(x0)
    B, C = x0.shape
    nb = len(weights) // 3
    cdt, dev = weights[0].dtype, x0.device
    t_codes = torch.empty((B, n_steps, C), dtype=torch.float32, device=dev)
    steps = max(n_steps - 1, 0)
    residuals = torch.empty((steps, nb, B, C), dtype=torch.float32, device=dev) if want_residuals else None
    xin = torch.empty((nb, steps, B, C), dtype=cdt, device=dev)
    h1 = torch.empty((nb, steps, B, H), dtype=cdt, device=dev)
    h2 = torch.empty((nb, steps, B, H), dtype=cdt, device=dev)
    lib = _lib.load_library()
    code = dtype_code(weights[0])
    parts = lib.vs_mlp_rollout_parts(code, B, C, H)
    Bp = (B + 15) // 16 * 16                 # sign-bit arrays: rows padded to whole 16-row slabs
    m1 = torch.empty((nb, steps, Bp, parts, 32), dtype=torch.int32, device=dev)
    m2 = torch.empty((nb, steps, Bp, parts, 32), dtype=torch.int32, device=dev)
    exchange_guard(dev)
    _probe_rollout_exchange(code, B, C, H, nb, dev)
    xws = _rollout_workspace(lib.vs_mlp_rollout_workspace_bytes(code, B, C, H), dev, (code, B, C, H))
    wa, ba = _ptr_array(weights), _ptr_array(biases)
    e0 = _pb()
    check(_lib.load_library().vs_mlp_rollout_fwd(dtype_code(weights[0]), B, C, H, nb, n_steps, x0.data_ptr(),
                                                 ctypes.cast(wa, ctypes.c_void_p), ctypes.cast(ba, ctypes.c_void_p),
                                                 t_codes.data_ptr(), _ptr(residuals), xin.data_ptr(), h1.data_ptr(),
                                                 h2.data_ptr(), m1.data_ptr(), m2.data_ptr(), _ptr(xws),
                                                 xws.numel() if xws is not None else 0, stream_ptr()),
          'vs_mlp_rollout_fwd')
    fl = 2.0 * B * steps * nb * (2 * C * H + H * H)
    _pe(e0, 'vs_mlp_rollout_fwd<%s>' % _DT[code_of(cdt)], flops=fl)
    return t_codes, residuals, (xin, h1, h2, m1, m2)


def mlp_rollout_bwd(grad_t_codes, weights_t, h1, h2, m1, m2, n_steps):
    """weights_t: packed [W3^T, W2^T, W1^T]*n_blocks (compute dtype).  Returns (dx0, dr, dh2, dh1)."""
    import ctypes
    require_cuda(grad_t_codes)
    B, n, C = grad_t_codes.shape
    nb = len(weights_t) // 3
    H = h1.shape[-1]
    cdt, dev = weights_t[0].dtype, grad_t_codes.device
    steps = max(n_steps - 1, 0)
    dx0 = torch.empty((B, C), dtype=torch.float32, device=dev)
    dr = torch.empty((nb, steps, B, C), dtype=cdt, device=dev)
    dh2 = torch.empty((nb, steps, B, H), dtype=cdt, device=dev)
    dh1 = torch.empty((nb, steps, B, H), dtype=cdt, device=dev)
    wa = _ptr_array(weights_t)
    lib = _lib.load_library()
    xws = _rollout_workspace(lib.vs_mlp_rollout_workspace_bytes(dtype_code(weights_t[0]), B, C, H), dev, (dtype_code(weights_t[0]), B, C, H))
    e0 = _pb()
    check(_lib.load_library().vs_mlp_rollout_bwd(dtype_code(weights_t[0]), B, C, H, nb, n_steps, grad_t_codes.data_ptr(),
                                                 ctypes.cast(wa, ctypes.c_void_p), h1.data_ptr(), h2.data_ptr(),
                                                 m1.data_ptr(), m2.data_ptr(), dx0.data_ptr(), dr.data_ptr(), dh2.data_ptr(), dh1.data_ptr(),
                                                 _ptr(xws), xws.numel() if xws is not None else 0, stream_ptr()),
          'vs_mlp_rollout_bwd')
    fl = 2.0 * B * steps * nb * (2 * C * H + H * H)
    _pe(e0, 'vs_mlp_rollout_bwd<%s>' % _DT[code_of(cdt)], flops=fl)
    return dx0, dr, dh2, dh1


# ------------------------------------------------------------------------------------------------ convolutions
def _conv_out_hw(H, W, k, stride, pad, transposed):
    if transposed:
        return (H - 1) * stride - 2 * pad + k, (W - 1) * stride - 2 * pad + k
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


_ConvGeom = collections.namedtuple('_ConvGeom', 'B Cin H W Cout k kw OH OW')


def _conv_geom(x_shape, w_shape, stride, pad, transposed):
    """The geometry of a (transposed) convolution call from its input and weight shapes, computed once per call."""
    B, Cin, H, W = x_shape
    k, kw = w_shape[2], w_shape[3]
    OH, OW = _conv_out_hw(H, W, k, stride, pad, transposed)
    return _ConvGeom(B, Cin, H, W, w_shape[1] if transposed else w_shape[0], k, kw, OH, OW)


def _wgrad_dest(into, out, w_shape, device):
    """Where a weight gradient goes: the pending gradient it is added to, the tensor that receives it, or a fresh fp32 tensor."""
    return into if into is not None else (out if out is not None else torch.empty(tuple(w_shape), dtype=torch.float32, device=device))


def conv_pack_weight(w_master, dtype, stride, pad, out=None):
    """fp32 master weight [D0, D1, k, k] -> packed operand of the transposed-form contractions (compute dtype)."""
    require_cuda(w_master)
    assert w_master.dtype == torch.float32 and w_master.is_contiguous()
    D0, D1, kh, kw = w_master.shape
    lib = _lib.load_library()
    if out is None:
        out = torch.empty((lib.vs_conv_packed_elems(D0, D1, kh, kw, stride, pad),), dtype=dtype, device=w_master.device)
    check(lib.vs_conv_pack_weight(code_of(dtype), w_master.data_ptr(), D0, D1, kh, kw, stride, pad,
                                  out.data_ptr(), stream_ptr()), 'vs_conv_pack_weight')
    return out


def _conv_workspace(x_dtype_code, B, Cin, H, W, Cout, k, stride, pad, device):
    """Transient column-matrix + split-K workspace of a convolution (VS_CONV_COLS=0: none -> gather inside the MFMA loop)."""
    if os.environ.get('VS_CONV_COLS') == '0':
        return None
    nbytes = _lib.load_library().vs_conv_workspace_bytes(x_dtype_code, B, Cin, H, W, Cout, k, k, stride, pad)
    return _workspace(nbytes, device) if nbytes else None


# ---- convolutions with 1..8 channels on the image side (csrc/vs_conv_thin.hip): dispatched from conv_fwd / conv_dgrad / conv_wgrad ----------
def _thin_plan(op, code, B, Cin, H, W, Cout, OH, OW, k, stride, pad, transposed, wgrad_max_m=8):
    """Whether this convolution call is one of the thin forms; returns (kind, C, Hb, Wb, M, sc, sm, flip) -- the many-channel map's channels and
    size, the thin channel count and how element (c, m, t) of the kernel's weight view is found in the weight tensor -- or None.
    The weight gradient takes its thin kernel up to `wgrad_max_m` thin channels (8 since round 4: no convolution of the BASELINE steps builds
    a column matrix any more.  With 4 / 5 / 8 thin channels -- the first encoder layers -- the column-matrix GEMM was the faster form, 57-72 us
    against 78-129 us: the VALU form re-reads the map per pair of thin channels)."""
    if code == F32 or pad != 1 or (k, stride) not in ((3, 1), (4, 2)):
        return None
    k2 = k * k
    plan = None
    if op == 'fwd':
        if not transposed and Cin <= 8 and (H, W) == (stride * OH, stride * OW):
            plan = ('expand', Cout, OH, OW, Cin, Cin * k2, k2, 0)
        elif not transposed and stride == 1 and Cout <= 4:
            plan = ('reduce', Cin, H, W, Cout, k2, Cin * k2, 1)
        elif transposed and Cout <= (4 if k == 3 else 2) and (OH, OW) == (stride * H, stride * W):
            plan = ('reduce', Cin, H, W, Cout, Cout * k2, k2, 0)
    elif op == 'dgrad':
        if transposed and Cout <= 8 and (OH, OW) == (stride * H, stride * W):
            plan = ('expand', Cin, H, W, Cout, Cout * k2, k2, 0)
        elif not transposed and stride == 1 and Cout <= 8:
            plan = ('expand', Cin, H, W, Cout, k2, Cin * k2, 1)
    else:
        if not transposed and Cin <= wgrad_max_m and (H, W) == (stride * OH, stride * OW):
            plan = ('wgrad_big_dy', Cout, OH, OW, Cin, Cin * k2, k2, 0)
        elif not transposed and stride == 1 and Cout <= wgrad_max_m:
            plan = ('wgrad_big_x', Cin, H, W, Cout, k2, Cin * k2, 1)
        elif transposed and Cout <= wgrad_max_m and (OH, OW) == (stride * H, stride * W):
            plan = ('wgrad_big_x', Cin, H, W, Cout, Cout * k2, k2, 0)
    if plan is None or not _lib.load_library().vs_conv_thin_supported(code, B, plan[1], plan[2], plan[3], plan[4], k, stride, pad):
        return None
    return plan


def conv_thin_expand(thin, w, bias, out_shape, out_dtype, k, stride, sc, sm, flip, role='fwd'):
    """out [B, C, H, W] = bias[c] + sum_{m, t} thin[B, M, S H, S W][m][S p + t - 1] * w(c, m, t)  (vs_conv_thin_expand)."""
    require_cuda(thin, w, bias)
    B, C, H, W = out_shape
    out = torch.empty(tuple(out_shape), dtype=out_dtype, device=thin.device)
    e0 = _pb()
    check(_lib.load_library().vs_conv_thin_expand(dtype_code(thin), thin.data_ptr(), w.data_ptr(), sc, sm, flip, _ptr(bias), out.data_ptr(), dtype_code(out),
                                                  B, C, H, W, thin.shape[1], k, stride, stream_ptr()), 'vs_conv_thin_expand')
    _pe(e0, 'vs_conv_thin:%s<%s>' % (role, _DT[dtype_code(thin)]), flops=2.0 * B * C * H * W * thin.shape[1] * k * k,
        nbytes=float(thin.numel() * thin.element_size() + out.numel() * out.element_size()))
    return out


def conv_thin_reduce(big, w, bias, M, out_dtype, k, stride, sc, sm, flip, role='fwd'):
    """out [B, M, S H, S W] = bias[m] + sum over the pixels / taps of big [B, C, H, W] that meet each output pixel  (vs_conv_thin_reduce)."""
    require_cuda(big, w, bias)
    B, C, H, W = big.shape
    out = torch.empty((B, M, stride * H, stride * W), dtype=out_dtype, device=big.device)
    e0 = _pb()
    check(_lib.load_library().vs_conv_thin_reduce(dtype_code(big), big.data_ptr(), w.data_ptr(), sc, sm, flip, _ptr(bias), out.data_ptr(), dtype_code(out),
                                                  B, C, H, W, M, k, stride, stream_ptr()), 'vs_conv_thin_reduce')
    _pe(e0, 'vs_conv_thin:%s<%s>' % (role, _DT[dtype_code(big)]), flops=2.0 * B * C * H * W * M * k * k,
        nbytes=float(big.numel() * big.element_size() + out.numel() * out.element_size()))
    return out


def conv_thin_wgrad(big, thin, w_shape, k, stride, sc, sm, flip, into=None, out=None):
    """dW (the weight's own layout, fp32) (+= into) = sum_{maps, p} big[c][p] * thin[m][S p + t - 1]  (vs_conv_thin_wgrad)."""
    require_cuda(big, thin)
    B, C, H, W = big.shape
    M = thin.shape[1]
    lib = _lib.load_library()
    dw = _wgrad_dest(into, out, w_shape, big.device)
    ws = _workspace(lib.vs_conv_thin_wgrad_workspace_bytes(B, C, H, W, M, k), big.device)
    e0 = _pb()
    check(lib.vs_conv_thin_wgrad(dtype_code(big), big.data_ptr(), thin.data_ptr(), ws.data_ptr(), ws.numel(), _ptr(into), dw.data_ptr(), sc, sm, flip,
                                 B, C, H, W, M, k, stride, stream_ptr()), 'vs_conv_thin_wgrad')
    _pe(e0, 'vs_conv_thin:wgrad<%s>' % _DT[dtype_code(big)], flops=2.0 * B * C * H * W * M * k * k,
        nbytes=float(big.numel() * big.element_size() + thin.numel() * thin.element_size() + dw.numel() * 4))
    return dw


# ---- ConvTranspose2d on a 1x1 map (the decoders' first_upconv, reference conv.py:258, 295: [B, C, 1, 1] -> [B, Cout, k, k]) IS a dense GEMM with
# the weight [Cin][Cout k k] as it lies in memory: no column matrix, no scatter ------------------------------------------------------------------
def _convt_1x1(x_shape, k, stride, pad, transposed):
    return transposed and x_shape[2] == 1 and x_shape[3] == 1 and pad == 0 and stride == 1


def _conv_full(x_shape, k, stride, pad, transposed):
    """Conv2d whose window is the whole (unpadded) map -- the encoders' `last_op` (reference conv.py:123, 169: Conv2d(8 nf, nh, 4, 1, 0) on a
    4 x 4 map -> 1 x 1): a Linear layer on the map as it lies in memory, y[b][co] = sum_j x[b][j] w[co][j], j = (ci, ky, kx).  No gather."""
    return not transposed and pad == 0 and x_shape[2] == k and x_shape[3] == k


def _conv_route(op, code, g, stride, pad, transposed):
    """The plain route of conv_fwd / conv_dgrad / conv_wgrad (`op`) with operands of type `code`: the first that holds of 'gemm_1x1', 'gemm_full',
    'thin', 'band_wgrad' (the weight gradient only) and 'cols', as (route, thin plan or None).  No side effects."""
    x_shape = (g.B, g.Cin, g.H, g.W)
    if _convt_1x1(x_shape, g.k, stride, pad, transposed):
        return 'gemm_1x1', None
    if _conv_full(x_shape, g.k, stride, pad, transposed) and g.kw == g.k:
        return 'gemm_full', None
    thin = _thin_plan(op, code, g.B, g.Cin, g.H, g.W, g.Cout, g.OH, g.OW, g.k, stride, pad, transposed) if g.kw == g.k else None
    if thin is not None:
        return 'thin', thin
    if op == 'wgrad' and not transposed and (g.k, stride, pad) == (3, 1, 1) and _wgrad_band_serves(code, g.B, g.Cin, g.H, g.W, g.Cout):
        return 'band_wgrad', None
    return 'cols', None


def _thin_conv(op, g, thin, big, w, bias, out_dtype, stride):
    """conv_fwd (big = x) / conv_dgrad (big = dy) on the thin kernel its plan names."""
    if thin[0] == 'expand':
        shape = (g.B, g.Cout, g.OH, g.OW) if op == 'fwd' else (g.B, g.Cin, g.H, g.W)
        return conv_thin_expand(big, w, bias, shape, out_dtype, g.k, stride, *thin[5:], role=op)
    return conv_thin_reduce(big, w, bias, g.Cout, out_dtype, g.k, stride, *thin[5:], role=op)


def _pe_cols(e0, op, g, transposed, tensors):
    """The profile entry of a column-matrix launch: its name, algorithmic FLOPs and the bytes of the three tensors it reads and writes."""
    work = g.B * g.Cin * g.H * g.W * g.Cout * g.k * g.k if transposed else g.B * g.Cout * g.OH * g.OW * g.Cin * g.k * g.k
    _pe(e0, 'vs_conv%s_cols:%s<%s>' % ('T' if transposed else '', op, _DT[dtype_code(tensors[0])]), flops=2.0 * work,
        nbytes=float(sum(t.numel() * t.element_size() for t in tensors)))


# ---- fp32 results from the 16-bit row-band kernels (VARSEP_FP32_SPLIT=1) ---------------------------------------------------------------------
# The row-band kernels take 16-bit operands, so the fp32 parity tests (1e-3 against the reference's fixture) ran the column-matrix route and
# never touched the kernels bench.py times.  A convolution is bilinear: with x = x0 + x1 + x2 and w = w0 + w1 + w2 (three bf16 pieces each: the
# bf16 head, the bf16 rounding of the remainder, and again -- 24 significant bits, i.e. the fp32 value exactly),
#   conv(x, w) = sum over i + j <= 2 of conv(x_i, w_j)  +  O(2^-24 |x| |w|):
# six launches of the SAME kernel (bf16 products are exact in the fp32 accumulator, fp32 output) reproduce the fp32 convolution to fp32
# rounding.  (Two pieces / three products leave 2^-16, which the VGG stack's per-call BatchNorms amplify to 1.3e-2 on the first BatchNorm
# weight's gradient: measured, above the 1e-2 bar.)  A test mode -- 6x the launches --, not a training mode.
_SPLIT_TERMS = ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))


def fp32_split_enabled():
    return os.environ.get('VARSEP_FP32_SPLIT', '0') == '1'


def _split16(t):
    parts, rest = [], t
    for _ in range(3):
        p = rest.to(torch.bfloat16)
        parts.append(p)
        rest = rest - p.float()
    return parts


def _split_route(op, g, fp32, stride, pad, transposed):
    """The fp32-split candidates of a call in the order they are tried -- the MFMA family of its geometry, then the thin kernels -- or none (not
    fp32 operands and result, or no VARSEP_FP32_SPLIT=1).  A candidate whose 16-bit kernel does not serve the shape falls to the next one, the
    last to the plain route."""
    if not (fp32 and fp32_split_enabled()):
        return ()
    family = ()
    if (g.k, g.kw, stride, pad) == (3, 3, 1, 1) and not transposed:
        family = ('conv3',)
    elif (g.k, g.kw, stride, pad) == (4, 4, 2, 1):
        # Conv2d forward and ConvTranspose2d input gradient gather the large map on its parity planes, the other two scatter (tap kernel)
        family = ('k4s2',) if op == 'wgrad' else ('gather',) if transposed == (op == 'dgrad') else ('tap',)
    return family + (('thin',) if g.k == g.kw else ())


def _split_sum(term, bias):
    """The six products term(i, j, bias) summed out of place (forward, input gradient): y = the first term, which takes the bias, then y.add_(t)."""
    y = None
    for i, j in _SPLIT_TERMS:
        t = term(i, j, bias if y is None else None)
        y = t if y is None else y.add_(t)
    return y


def _split_chain(term, into, out):
    """The six products term(i, j, into, out) of a weight gradient, summed by the launches themselves: the first goes to `into` / `out` / a fresh
    tensor, every later one is added to that."""
    dw = None
    for i, j in _SPLIT_TERMS:
        dw = term(i, j, into if dw is None else dw, out if dw is None else None)
    return dw


def _tap_f32(x, w_tap, bias, Cout, role):
    """ConvTranspose2d k4 s2 p1 of 16-bit x through the tap kernel with fp32 output (the Conv2d input gradient is the same operation on dy)."""
    B, Cin, H, W = x.shape
    t = torch.empty((B, Cout, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    e0 = _pb()
    check(_lib.load_library().vs_convt_k4s2_tap_fwd_f32(_lib.BF16, x.data_ptr(), w_tap.data_ptr(), _ptr(bias), t.data_ptr(), B, Cin, H, W, Cout, stream_ptr()),
          'vs_convt_k4s2_tap_fwd_f32')
    _pe(e0, 'vs_convT_tap:%s<bf16>' % role, flops=2.0 * B * H * W * Cin * Cout * 16, nbytes=float(x.numel() * 2 + t.numel() * 4))
    return t


def _conv_split(op, g, big, w, bias, fp32, stride, pad, transposed):
    """fp32 conv_fwd (big = x) / conv_dgrad (big = dy, no bias) as six launches of a 16-bit kernel on the pieces (bs[i], ws[j]); None when no
    split candidate serves the call.  M: the channels of the result."""
    M = g.Cout if op == 'fwd' else g.Cin
    for name in _split_route(op, g, fp32, stride, pad, transposed):
        if name == 'thin':
            # the thin-channel edge layers (first encoder / last decoder convolution): the same six products on the VALU kernels
            thin = _thin_plan(op, BF16, g.B, g.Cin, g.H, g.W, g.Cout, g.OH, g.OW, g.k, stride, pad, transposed)
            if thin is None:
                continue
            bs, ws = _split16(big), _split16(w)
            term = lambda i, j, b: _thin_conv(op, g, thin, bs[i], ws[j], b, torch.float32, stride)
        elif name == 'conv3':
            # Conv2d k3 s1 p1 (its input gradient: w [Cout, Cin, 3, 3] applied flipped) on the row-band kernel
            bs = _split16(big)
            few = conv3_img16_supported(bs[0], M)            # the SST integrator's few 16 x 16 maps: the few-maps kernel (same weight pre-pack)
            if not few and not conv3_band_supported(bs[0], M):
                continue
            ws = [conv3_img16_pack_weight(p.float().contiguous(), torch.bfloat16, op == 'dgrad') for p in _split16(w)]
            if few:
                term = lambda i, j, b: slab_sum(conv3_img16(bs[i], ws[j], M, role=op), b, torch.float32)
            else:
                term = lambda i, j, b: conv3_band(bs[i], ws[j], b, M, torch.float32, role=op)
        elif name == 'gather':
            # k4 s2 p1 gather (Conv2d forward on x / ConvTranspose2d input gradient on dy; w [M, K, 4, 4]) on the parity planes
            bs = _split16(big)
            if not conv_k4s2_gather_supported(bs[0], M):
                continue
            planes = [space_to_depth2(b) for b in bs]
            ws = [conv_k4s2_pack_weight(p.float().contiguous(), torch.bfloat16) for p in _split16(w)]
            term = lambda i, j, b: conv_k4s2_gather(planes[i], ws[j], b, M, torch.float32, role=op)
        else:
            # k4 s2 p1 SCATTER (ConvTranspose2d forward of x with w [Cin, Cout, 4, 4]; the input gradient of a Conv2d is the same operation on
            # dy with its weight [Cout, Cin, 4, 4] read as [in = Cout, out = Cin]) on the tap kernel
            bs = _split16(big)
            if not convt_tap_supported(bs[0], M, 1):
                continue
            ws = [convt_tap_pack_weight(p.float().contiguous(), torch.bfloat16) for p in _split16(w)]
            term = lambda i, j, b: _tap_f32(bs[i], ws[j], b, M, op)
        return _split_sum(term, bias)
    return None


def _wgrad_split(g, dy, x, w_shape, stride, pad, transposed, into, out):
    """fp32 conv_wgrad as six launches of a 16-bit kernel, accumulated by the kernels' own finishing pass (`into`); None when no split
    candidate serves the call.  dW is bilinear in (dy, x): the same six products."""
    for name in _split_route('wgrad', g, x.dtype == torch.float32, stride, pad, transposed):
        if name == 'conv3':
            xs = _split16(x)
            if not conv3_wgrad_band_supported(xs[0], g.Cout):
                continue
            ds = _split16(dy)
            term = lambda i, j, into_, out_: conv_wgrad(ds[j], xs[i], w_shape, stride, pad, transposed, into=into_, out=out_)
        elif name == 'k4s2':
            # k4 s2 p1: the LARGE map (x of a Conv2d, dy of a ConvTranspose2d) on its parity planes, the small one as it is
            big, small = (dy, x) if transposed else (x, dy)
            bs = _split16(big)
            if not conv_k4s2_supported(bs[0], w_shape[0]):
                continue
            planes = [space_to_depth2(b) for b in bs]
            ss = _split16(small)
            term = lambda i, j, into_, out_: conv_k4s2_wgrad(ss[j], planes[i], w_shape, into=into_, out=out_)
        else:
            thin = _thin_plan('wgrad', BF16, g.B, g.Cin, g.H, g.W, g.Cout, g.OH, g.OW, g.k, stride, pad, transposed)
            if thin is None:
                continue
            big, small = (dy, x) if thin[0] == 'wgrad_big_dy' else (x, dy)
            bs, ss = _split16(big), _split16(small)
            term = lambda i, j, into_, out_: conv_thin_wgrad(bs[i], ss[j], w_shape, g.k, stride, *thin[5:], into=into_, out=out_)
        return _split_chain(term, into, out)
    return None


def conv_fwd(x, w, bias, stride, pad, transposed, out_dtype, w_packed=None):
    """x [B,Cin,H,W], w Conv2d [Cout,Cin,k,k] / ConvTranspose2d [Cin,Cout,k,k] in the same (compute) dtype.
    The transposed form consumes `w_packed` (conv_pack_weight); it is built on the fly from `w` when not given."""
    require_cuda(x, w, bias)
    assert x.is_contiguous() and w.is_contiguous() and x.dtype == w.dtype
    g = _conv_geom(x.shape, w.shape, stride, pad, transposed)
    y = _conv_split('fwd', g, x, w, bias, x.dtype == torch.float32 and out_dtype == torch.float32, stride, pad, transposed)
    if y is not None:
        return y
    if transposed and w_packed is None:
        w_packed = conv_pack_weight(w.float().contiguous(), x.dtype, stride, pad)
    route, thin = _conv_route('fwd', dtype_code(x), g, stride, pad, transposed)
    B, Cin, H, W, Cout, k, kw, OH, OW = g
    if route == 'gemm_1x1':
        # y[b][(co, ky, kx)] = sum_ci x[b][ci] w[ci][(co, ky, kx)] + bias[co]
        n = Cout * k * kw
        brep = bias.repeat_interleave(k * kw) if bias is not None else None
        y = gemm(x.view(B, Cin), LAYOUT_R, w.view(Cin, n), LAYOUT_S, B, n, Cin, out_dtype=out_dtype, bias=brep)
        return y.view(B, Cout, k, kw)
    if route == 'gemm_full':
        n = Cin * k * k
        return gemm(x.view(B, n), LAYOUT_R, w.view(Cout, n), LAYOUT_R, B, Cout, n, out_dtype=out_dtype, bias=bias).view(B, Cout, 1, 1)
    if route == 'thin':
        return _thin_conv('fwd', g, thin, x, w, bias, out_dtype, stride)
    y = torch.empty((B, Cout, OH, OW), dtype=out_dtype, device=x.device)
    lib = _lib.load_library()
    fn = lib.vs_conv_transpose2d_fwd if transposed else lib.vs_conv2d_fwd
    ws = _conv_workspace(dtype_code(x), B, Cin, H, W, Cout, k, stride, pad, x.device)
    e0 = _pb()
    check(fn(dtype_code(x), x.data_ptr(), (w_packed if transposed else w).data_ptr(), _ptr(bias), y.data_ptr(), dtype_code(y), B, Cin, H, W, Cout, k, k,
             stride, pad, _ptr(ws), ws.numel() if ws is not None else 0, stream_ptr()), 'vs_conv_fwd')
    _pe_cols(e0, 'fwd', g, transposed, (x, w, y))
    return y


def conv_dgrad(dy, w, x_shape, stride, pad, transposed, out_dtype, w_packed=None, cols_from_wgrad=False):
    """cols_from_wgrad (ConvTranspose2d only): conv_wgrad of the same dy / geometry ran just before on this stream, reuse its column
    matrix instead of gathering dy a second time."""
    require_cuda(dy, w)
    assert dy.is_contiguous() and w.is_contiguous() and dy.dtype == w.dtype
    g = _conv_geom(x_shape, w.shape, stride, pad, transposed)
    assert tuple(dy.shape[2:]) == (g.OH, g.OW), (tuple(dy.shape), g)
    dx = _conv_split('dgrad', g, dy, w, None, dy.dtype == torch.float32 and out_dtype == torch.float32, stride, pad, transposed)
    if dx is not None:
        return dx
    if not transposed and w_packed is None:
        w_packed = conv_pack_weight(w.float().contiguous(), dy.dtype, stride, pad)
    route, thin = _conv_route('dgrad', dtype_code(dy), g, stride, pad, transposed)
    B, Cin, H, W, Cout, k, kw, OH, OW = g
    if route == 'gemm_1x1':
        # dx[b][ci] = sum_j dy[b][j] w[ci][j], j = (co, ky, kx)
        n = Cout * k * kw
        return gemm(dy.view(B, n), LAYOUT_R, w.view(Cin, n), LAYOUT_R, B, Cin, n, out_dtype=out_dtype).view(B, Cin, 1, 1)
    if route == 'gemm_full':
        # dx[b][j] = sum_co dy[b][co] w[co][j]
        n = Cin * k * k
        return gemm(dy.view(B, Cout), LAYOUT_R, w.view(Cout, n), LAYOUT_S, B, n, Cout, out_dtype=out_dtype).view(B, Cin, k, k)
    if route == 'thin':
        return _thin_conv('dgrad', g, thin, dy, w, None, out_dtype, stride)
    dx = torch.empty((B, Cin, H, W), dtype=out_dtype, device=dy.device)
    lib = _lib.load_library()
    fn = lib.vs_conv_transpose2d_dgrad if transposed else lib.vs_conv2d_dgrad
    ws = _conv_workspace(dtype_code(dy), B, Cin, H, W, Cout, k, stride, pad, dy.device)
    e0 = _pb()
    extra = (int(bool(cols_from_wgrad)),) if transposed else ()
    check(fn(dtype_code(dy), dy.data_ptr(), (w if transposed else w_packed).data_ptr(), dx.data_ptr(), dtype_code(dx), B, Cin, H, W, Cout, k, k, stride, pad,
             _ptr(ws), ws.numel() if ws is not None else 0, *extra, stream_ptr()), 'vs_conv_dgrad')
    _pe_cols(e0, 'dgrad', g, transposed, (dy, w, dx))
    return dx


def _wgrad_band_serves(code, B, Cin, H, W, Cout):
    """Whether the row-band kernel serves the weight gradient of Conv2d k3 s1 p1 on 16-bit maps [B, Cin, H, W].  VS_CONV_WGRAD_BAND=0: never."""
    if os.environ.get('VS_CONV_WGRAD_BAND') == '0' or code == F32 or (Cin * Cout * 9) % 4 != 0:
        return False
    return bool(_lib.load_library().vs_conv3_wgrad_band_supported(code, B, Cin, H, W, Cout))


def conv3_wgrad_band_supported(x, Cout, dtype_code_of=None):
    """Whether the weight gradient of Conv2d k3 s1 p1 with input `x` takes the row-band kernel (no column matrix).  VS_CONV_WGRAD_BAND=0: never.
    (`x` may be a meta tensor that only carries the shape; then `dtype_code_of` is the operand type code.)"""
    if x.dtype == torch.float32 or x.dim() != 4:
        return False
    return _wgrad_band_serves(dtype_code_of if dtype_code_of is not None else dtype_code(x), *x.shape, Cout)


def _slab_reduce(slabs, nslabs, w_shape, into, dw, finish='vs_conv3_wgrad_band_finish'):
    """dw = sum of `nslabs` fp32 partial gradients (+ the pending gradient `into`); two passes when a small weight has many slabs."""
    lib = _lib.load_library()
    src, n = slabs, nslabs
    if nslabs > 24:
        # many slabs of a small weight: a first pass in 16 groups (every workgroup adds <= nslabs / 16 coalesced slabs), then the 16 partials
        src = torch.empty((16,) + tuple(slabs.shape[1:]), dtype=torch.float32, device=slabs.device)
        check(lib.vs_slab_sum_grouped(slabs.data_ptr(), nslabs, 16, src.data_ptr(), slabs.numel() // nslabs, stream_ptr()), 'vs_slab_sum_grouped')
        n = -(-nslabs // (-(-nslabs // 16)))          # groups that received slabs: ceil(nslabs / per)
    # the slabs are laid out [tap][Cout][Cin] (coalesced stores in the kernel): the last pass transposes into the weight's own layout
    check(getattr(lib, finish)(src.data_ptr(), n, _ptr(into), dw.data_ptr(), w_shape[0], w_shape[1], stream_ptr()), finish)


def _wgrad_band(launch, code, B, Cin, H, W, w_shape, into, dw, operand_bytes):
    """3x3 on maps of width 4 .. 64: row bands in LDS, no column matrix; `launch(lib, slabs pointer)` leaves partial gradients in slabs, one
    (or two) launches add them into dw."""
    lib = _lib.load_library()
    nslabs = lib.vs_conv3_wgrad_band_slabs(B, Cin, H, W, w_shape[0])
    slabs = torch.empty((nslabs,) + tuple(w_shape), dtype=torch.float32, device=dw.device)
    e0 = _pb()
    launch(lib, slabs.data_ptr())
    _slab_reduce(slabs, nslabs, w_shape, into, dw)
    _pe(e0, 'vs_conv3_wgrad_band<%s>' % _DT[code], flops=2.0 * B * w_shape[0] * H * W * Cin * 9, nbytes=float(operand_bytes + slabs.numel() * 8))
    return dw


def conv3_wgrad_band_pieces(pairs, w_shape, into=None):
    """Weight gradient of Conv2d k3 s1 p1 over the batch formed by the (dz, x) pairs -- equal shapes, each contiguous -- WITHOUT concatenating
    them (`vs_conv3_wgrad_band_pieces`: the piece pointers travel as kernel arguments).  Returns None when the row-band kernel does not
    serve the concatenated shape or there are more than 64 pieces (the caller concatenates)."""
    import ctypes
    dz0, x0 = pairs[0]
    n = len(pairs)
    mp, Cin, H, W = x0.shape
    Cout = w_shape[0]
    if (W == 8 and mp % 4 != 0) or (W == 4 and mp % 16 != 0) or n > 64 or any(p[0].shape != dz0.shape or p[1].shape != x0.shape or not p[0].is_contiguous() or not p[1].is_contiguous()
                     or p[0].dtype != x0.dtype or p[1].dtype != x0.dtype for p in pairs):
        return None
    if not _wgrad_band_serves(dtype_code(x0), n * mp, Cin, H, W, Cout):
        return None
    xs = (ctypes.c_void_p * n)(*[p[1].data_ptr() for p in pairs])
    dzs = (ctypes.c_void_p * n)(*[p[0].data_ptr() for p in pairs])
    return _wgrad_band(lambda lib, slabs: check(lib.vs_conv3_wgrad_band_pieces(dtype_code(x0), n, xs, dzs, mp, slabs, Cin, H, W, Cout, stream_ptr()),
                                                'vs_conv3_wgrad_band_pieces'),
                       dtype_code(x0), n * mp, Cin, H, W, w_shape, into, _wgrad_dest(into, None, w_shape, x0.device),
                       n * (dz0.numel() + x0.numel()) * x0.element_size())


def conv_wgrad(dy, x, w_shape, stride, pad, transposed, into=None, out=None):
    """Weight gradient of a (transposed) convolution; `into`: an fp32 tensor of the weight's shape that the result is ADDED to
    (in the GEMM / split-K epilogue) instead of a fresh tensor; `out`: an fp32 tensor that receives it."""
    require_cuda(dy, x)
    assert dy.is_contiguous() and x.is_contiguous() and dy.dtype == x.dtype
    g = _conv_geom(x.shape, w_shape, stride, pad, transposed)
    assert tuple(dy.shape[2:]) == (g.OH, g.OW), (tuple(dy.shape), g)
    if into is not None:
        assert into.dtype == torch.float32 and into.is_contiguous() and tuple(into.shape) == tuple(w_shape)
    if out is not None:
        assert into is None and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == tuple(w_shape)
    dw = _wgrad_split(g, dy, x, w_shape, stride, pad, transposed, into, out)
    if dw is not None:
        return dw
    route, thin = _conv_route('wgrad', dtype_code(x), g, stride, pad, transposed)
    B, Cin, H, W, Cout, k, kw, OH, OW = g
    if route == 'thin':
        big, small = (dy, x) if thin[0] == 'wgrad_big_dy' else (x, dy)
        return conv_thin_wgrad(big, small, w_shape, k, stride, *thin[5:], into=into, out=out)
    dw = _wgrad_dest(into, out, w_shape, x.device)
    if route == 'gemm_1x1':
        # dW[ci][j] (+)= sum_b x[b][ci] dy[b][j]
        n = Cout * k * kw
        gemm(x.view(B, Cin), LAYOUT_S, dy.view(B, n), LAYOUT_S, Cin, n, B, out=dw.view(Cin, n), accumulate=into is not None)
    elif route == 'gemm_full':
        # dW[co][j] (+)= sum_b dy[b][co] x[b][j]
        n = Cin * k * k
        gemm(dy.view(B, Cout), LAYOUT_S, x.view(B, n), LAYOUT_S, Cout, n, B, out=dw.view(Cout, n), accumulate=into is not None)
    elif route == 'band_wgrad':
        _wgrad_band(lambda lib, slabs: check(lib.vs_conv3_wgrad_band(dtype_code(x), x.data_ptr(), dy.data_ptr(), slabs, B, Cin, H, W, Cout, stream_ptr()),
                                             'vs_conv3_wgrad_band'),
                    dtype_code(x), B, Cin, H, W, w_shape, into, dw, (dy.numel() + x.numel()) * x.element_size())
    else:
        lib = _lib.load_library()
        ws = _conv_workspace(dtype_code(x), B, Cin, H, W, Cout, k, stride, pad, x.device)
        if ws is None:
            pix_h, pix_w = (H, W) if transposed else (OH, OW)
            ws_bytes = lib.vs_conv_wgrad_workspace_bytes(B, Cin, pix_h, pix_w, Cout, k, k)
            ws = _workspace(ws_bytes, x.device) if ws_bytes else None
        fn = lib.vs_conv_transpose2d_wgrad_acc if transposed else lib.vs_conv2d_wgrad_acc
        e0 = _pb()
        check(fn(dtype_code(x), dy.data_ptr(), x.data_ptr(), dw.data_ptr(), B, Cin, H, W, Cout, k, k, stride, pad, _ptr(ws),
                 ws.numel() if ws is not None else 0, 1 if into is not None else 0, stream_ptr()), 'vs_conv_wgrad')
        _pe_cols(e0, 'wgrad', g, transposed, (dy, x, dw))
    return dw


# ---- 4x4 stride-2 pad-1 convolutions on the parity planes of their input (csrc/vs_conv_k4s2.hip) --------------------------------
def conv_k4s2_supported(big, M):
    """Whether the gather-type operations of a k4 s2 p1 (transposed) convolution on the LARGE map `big` [B, C, H, W] -- Conv2d forward /
    weight gradient (big = the input, M = Cout), ConvTranspose2d input / weight gradient (big = the output gradient, M = Cin) -- run on
    the parity planes of `big` with the row-band kernels (no column matrix)."""
    if not conv_k4s2_gather_supported(big, M):
        return False
    B, C, H, W = big.shape
    return bool(_lib.load_library().vs_conv3_wgrad_band_supported(dtype_code(big), B, 4 * C, H // 2, W // 2, M))


def conv_k4s2_gather_supported(big, M):
    """`conv_k4s2_supported` for the GATHER alone (Conv2d forward / ConvTranspose2d input gradient on the parity planes): 8 x 8 maps have 4 x 4
    planes, which the row-band forward kernel serves (sixteen maps per workgroup) but the row-band weight gradient does not."""
    if big.dtype == torch.float32 or big.dim() != 4:
        return False
    B, C, H, W = big.shape
    lib = _lib.load_library()
    code = dtype_code(big)
    return (C % 16 == 0 and bool(lib.vs_space_to_depth2_supported(code, B, C, H, W))       # (the plane pre-packs hold whole 64-channel phases)
            and bool(lib.vs_conv3_band_supported(code, B, 4 * C, H // 2, W // 2, M)))


def space_to_depth2(x):
    """x [B, C, H, W] (16-bit) -> its four parity planes [B, 4 C, H/2, W/2], channel = (row parity * 2 + column parity) * C + c."""
    require_cuda(x)
    assert x.is_contiguous()
    B, C, H, W = x.shape
    y = torch.empty((B, 4 * C, H // 2, W // 2), dtype=x.dtype, device=x.device)
    e0 = _pb()
    check(_lib.load_library().vs_space_to_depth2(dtype_code(x), x.data_ptr(), y.data_ptr(), B, C, H, W, stream_ptr()), 'vs_space_to_depth2')
    _pe(e0, 'vs_space_to_depth2', nbytes=float(2 * x.numel() * x.element_size()))
    return y


def conv_k4s2_pack_weight(w_master, dtype, out=None):
    """fp32 [M, K, 4, 4] -> the row-band kernels' pre-pack over the 4 K plane channels (vs_conv_k4s2_pack_weight)."""
    require_cuda(w_master)
    assert w_master.dtype == torch.float32 and w_master.is_contiguous() and tuple(w_master.shape[2:]) == (4, 4)
    M, K = w_master.shape[0], w_master.shape[1]
    lib = _lib.load_library()
    if out is None:
        out = torch.empty((lib.vs_conv_k4s2_packed_elems(K, M),), dtype=dtype, device=w_master.device)
    check(lib.vs_conv_k4s2_pack_weight(code_of(dtype), w_master.data_ptr(), K, M, out.data_ptr(), stream_ptr()), 'vs_conv_k4s2_pack_weight')
    return out


def conv_k4s2_gather(planes, w_packed, bias, M, out_dtype, role='fwd', bn_sums=None, groups=1):
    """out [B, M, h, w] = k4 s2 p1 gather of the large map whose parity planes are `planes` [B, 4 K, h, w] with the packed weight
    (Conv2d forward: role 'fwd'; ConvTranspose2d input gradient: role 'dgrad')."""
    require_cuda(planes, w_packed, bias)
    assert planes.is_contiguous() and planes.dtype == w_packed.dtype
    B, C4, H, W = planes.shape
    y = torch.empty((B, M, H, W), dtype=out_dtype, device=planes.device)
    e0 = _pb()
    check(_lib.load_library().vs_conv_k4s2_band_bn(dtype_code(planes), planes.data_ptr(), w_packed.data_ptr(), _ptr(bias), y.data_ptr(), dtype_code(y), B,
                                                   C4 // 4, H, W, M, _ptr(bn_sums), groups, stream_ptr()), 'vs_conv_k4s2_band')
    # algorithmic work of the 4x4 window: 16 taps x K channels (the zero taps of the 3x3 form are not counted)
    _pe(e0, 'vs_conv_k4s2:%s<%s>' % (role, _DT[dtype_code(planes)]), flops=2.0 * B * H * W * M * (C4 // 4) * 16,
        nbytes=float(planes.numel() * planes.element_size() + M * (C4 // 4) * 16 * 2 + y.numel() * y.element_size()))
    return y


def conv_k4s2_wgrad(small, planes, w_shape, into=None, out=None):
    """dW [M, K, 4, 4] (fp32) of a k4 s2 p1 (transposed) convolution from the SMALL map `small` [B, M, h, w] and the parity planes of the
    large one [B, 4 K, h, w]; `into`: ADDED to this pending gradient, `out`: written there."""
    require_cuda(small, planes)
    assert small.is_contiguous() and planes.is_contiguous() and small.dtype == planes.dtype
    B, M, H, W = small.shape
    K = planes.shape[1] // 4
    assert tuple(w_shape) == (M, K, 4, 4), (tuple(w_shape), M, K)
    lib = _lib.load_library()
    dw = _wgrad_dest(into, out, w_shape, small.device)
    assert dw.dtype == torch.float32 and dw.is_contiguous() and tuple(dw.shape) == tuple(w_shape)
    nslabs = lib.vs_conv_k4s2_wgrad_band_slabs(B, K, H, W, M)
    n3 = M * 4 * K * 9
    slabs = torch.empty((nslabs, n3), dtype=torch.float32, device=small.device)
    e0 = _pb()
    check(lib.vs_conv_k4s2_wgrad_band(dtype_code(planes), planes.data_ptr(), small.data_ptr(), slabs.data_ptr(), B, K, H, W, M, stream_ptr()),
          'vs_conv_k4s2_wgrad_band')
    _slab_reduce(slabs, nslabs, w_shape, into, dw, finish='vs_conv_k4s2_wgrad_finish')
    _pe(e0, 'vs_conv_k4s2:wgrad<%s>' % _DT[dtype_code(planes)], flops=2.0 * B * H * W * M * K * 16,
        nbytes=float(small.numel() * small.element_size() + planes.numel() * planes.element_size() + slabs.numel() * 8))
    return dw


# ---- ConvTranspose2d k4 s2 p1 forward as tap GEMM + col2im epilogue (csrc/vs_conv_tap.hip) -------------------------------------
def convt_tap_supported(x, Cout, groups):
    if x.dtype == torch.float32:
        return False
    B, Cin, H, W = x.shape
    return bool(_lib.load_library().vs_convt_tap_supported(dtype_code(x), B, Cin, H, W, Cout, groups))


def convt_tap_pack_weight(w_master, dtype, out=None):
    """fp32 ConvTranspose2d weight [Cin, Cout, 4, 4] -> [ceil(Cout/16), 16 taps x 16 channels, Cin] in `dtype`."""
    require_cuda(w_master)
    assert w_master.dtype == torch.float32 and w_master.is_contiguous() and tuple(w_master.shape[2:]) == (4, 4)
    Cin, Cout = w_master.shape[0], w_master.shape[1]
    lib = _lib.load_library()
    if out is None:
        out = torch.empty((lib.vs_convt_tap_packed_elems(Cin, Cout),), dtype=dtype, device=w_master.device)
    check(lib.vs_convt_tap_pack_weight(code_of(dtype), w_master.data_ptr(), Cin, Cout, out.data_ptr(), stream_ptr()), 'vs_convt_tap_pack_weight')
    return out


def convt_tap_fwd(x, w_tap, bias, Cout, groups=1, want_sums=True, role='fwd'):
    """-> (y [B, Cout, 2H, 2W] in x's dtype, fp64 sums [groups, Cout, 2] of the stored outputs or None)."""
    require_cuda(x, w_tap, bias)
    assert x.is_contiguous() and x.dtype == w_tap.dtype
    B, Cin, H, W = x.shape
    y = torch.empty((B, Cout, 2 * H, 2 * W), dtype=x.dtype, device=x.device)
    sums = torch.empty((groups, Cout, 2), dtype=torch.float64, device=x.device) if want_sums else None
    e0 = _pb()
    check(_lib.load_library().vs_convt_k4s2_tap_fwd(dtype_code(x), x.data_ptr(), w_tap.data_ptr(), _ptr(bias), y.data_ptr(), _ptr(sums), B, Cin, H, W,
                                                    Cout, groups, stream_ptr()), 'vs_convt_k4s2_tap_fwd')
    _pe(e0, 'vs_convT_tap:%s<%s>' % (role, _DT[dtype_code(x)]), flops=2.0 * B * Cin * H * W * Cout * 16,
        nbytes=float(x.numel() * x.element_size() + w_tap.numel() * 2 + y.numel() * y.element_size()))
    return y, sums


def conv_k3_tap_supported(x, Cout, groups, force=False):
    """Whether Conv2d k3 s1 p1 on `x` takes the tap kernel.  Measured (tools/conv_bench.py): with 9 taps x 28 channels per tile the
    epilogue (shift-sum of nine maps) outweighs the saved column matrix unless the contraction is long -- 512 -> 512 at 16x16
    (the SST integrator): 45 vs 65 us; 128 -> 128 (K = 4 tiles): 489 vs 371 us -- so it is taken for Cin >= 384, Cout >= 256
    (force=True: whenever the geometry is supported)."""
    if x.dtype == torch.float32:
        return False
    B, Cin, H, W = x.shape
    if not force and (Cin < 384 or Cout < 256):
        return False
    return bool(_lib.load_library().vs_conv_k3_tap_supported(dtype_code(x), B, Cin, H, W, Cout, groups))


def conv3_img16_supported(x, Cout):
    """Whether Conv2d k3 s1 p1 on `x` takes the few-images kernel (`conv3_img16`): 16x16 maps, 16-bit, Cin a multiple of 64 and a batch
    small enough that the per-image tiling pays (the SST integrator: 8 maps)."""
    if x.dtype == torch.float32 or x.dim() != 4:
        return False
    B, Cin, H, W = x.shape
    if B > 32:
        return False
    return bool(_lib.load_library().vs_conv3_img16_supported(dtype_code(x), B, Cin, H, W, Cout))


def conv3_img16_pack_weight(w_master, dtype, flip, out=None):
    """fp32 Conv2d weight [Cout, Cin, 3, 3] -> MFMA-fragment order for `conv3_img16` in `dtype`.  flip=False: forward (rows = Cout,
    contraction = Cin); flip=True: input gradient (rows = Cin, contraction = Cout, taps flipped)."""
    require_cuda(w_master)
    assert w_master.dtype == torch.float32 and w_master.is_contiguous() and tuple(w_master.shape[2:]) == (3, 3)
    Cout, Cin = w_master.shape[0], w_master.shape[1]
    M, K = (Cin, Cout) if flip else (Cout, Cin)
    lib = _lib.load_library()
    if out is None:
        out = torch.empty((lib.vs_conv3_img16_packed_elems(K, M),), dtype=dtype, device=w_master.device)
    check(lib.vs_conv3_img16_pack_weight(code_of(dtype), w_master.data_ptr(), K, M, int(bool(flip)), out.data_ptr(), stream_ptr()),
          'vs_conv3_img16_pack_weight')
    return out


def conv3_img16_pack_weights(jobs, dtype):
    """jobs = [(w_master fp32 [Cout, Cin, 3, 3] contiguous, flip, out buffer or None)] -> list of packed buffers, ONE launch per 96 jobs."""
    import ctypes
    lib = _lib.load_library()
    outs = []
    for w, flip, buf in jobs:
        Cout, Cin = w.shape[0], w.shape[1]
        M, K = (Cin, Cout) if flip else (Cout, Cin)
        if buf is None:
            buf = torch.empty((lib.vs_conv3_img16_packed_elems(K, M),), dtype=dtype, device=w.device)
        outs.append((w, int(bool(flip)), buf, M, K))
    for i in range(0, len(outs), 96):
        chunk = outs[i:i + 96]
        n = len(chunk)
        VP, I32 = ctypes.c_void_p * n, ctypes.c_int32 * n
        check(lib.vs_conv3_img16_pack_weights(code_of(dtype), n, VP(*[c[0].data_ptr() for c in chunk]), I32(*[c[4] for c in chunk]),
                                              I32(*[c[3] for c in chunk]), I32(*[c[1] for c in chunk]), VP(*[c[2].data_ptr() for c in chunk]),
                                              stream_ptr()), 'vs_conv3_img16_pack_weights')
    return [c[2] for c in outs]


def conv3_img16(x, w_packed, Cout, role='fwd'):
    """Conv2d k3 s1 p1 of x [B, Cin, 16, 16] -> fp32 split slabs [S, B, Cout, 16, 16] WITHOUT bias (S = vs_conv3_img16_splits); consumers:
    `bn_train_fwd_small_slabs`, `slab_sum`."""
    require_cuda(x, w_packed)
    assert x.is_contiguous() and x.dtype == w_packed.dtype
    B, Cin, H, W = x.shape
    lib = _lib.load_library()
    S = lib.vs_conv3_img16_splits(B, Cin, Cout)
    slabs = torch.empty((S, B, Cout, H, W), dtype=torch.float32, device=x.device)
    e0 = _pb()
    check(lib.vs_conv3_img16(dtype_code(x), x.data_ptr(), w_packed.data_ptr(), slabs.data_ptr(), B, Cin, Cout, stream_ptr()), 'vs_conv3_img16')
    _pe(e0, 'vs_conv3_img16:%s<%s>' % (role, _DT[dtype_code(x)]), flops=2.0 * B * Cin * H * W * Cout * 9,
        nbytes=float(x.numel() * x.element_size() + w_packed.numel() * 2 + slabs.numel() * 4))
    return slabs


def conv3_band_supported(x, Cout):
    """Whether Conv2d k3 s1 p1 on `x` takes the row-band kernel (`conv3_band`: many maps of width 4 / 8 / 16 / 32 / 64, any channel count --
    a last 64-channel phase is filled with zeros --, no column matrix).  Below 16 channels on either side the thin-channel kernels (one VALU
    pass, no 32 x 64-wide MFMA tiles of padding) keep the layer."""
    if x.dtype == torch.float32 or x.dim() != 4:
        return False
    B, Cin, H, W = x.shape
    if Cin < 16 or Cout < 16:
        return False
    return bool(_lib.load_library().vs_conv3_band_supported(dtype_code(x), B, Cin, H, W, Cout))


# ---- BatchNorm sums taken in a convolution's epilogue: persistent fp64 buffers [groups, C, 2], zero between steps (vs_bn_stats_from_sums_fold
# resets what it has read, so no fill launch is needed per convolution) ----------------------------------------------------------------------
_BN_SUMS = {}


def bn_sums_buffer(key, groups, C, device):
    """The persistent sums buffer of one BatchNorm call site (`key`: e.g. the data pointer of its running mean), zero-filled when created."""
    k = (device.index, key, groups, C)
    buf = _BN_SUMS.get(k)
    if buf is None:
        buf = _BN_SUMS[k] = torch.zeros((groups, C, 2), dtype=torch.float64, device=device)
    return buf


def band_bn_mode():
    """How the row-band kernels leave the BatchNorm statistics of their output (VS_BAND_BN_SUMS): '0' (default: a statistics pass over the
    stored output), 'parts' (round 4: per-workgroup partial sums in a table + a fold launch, no atomics, reproducible), '1' (round 3: fp64
    atomics).  Both epilogue forms are MEASURED SLOWER than the pass they replace and stay opt-in: the pass reads the 16-bit tensor once at
    HBM rate (11-80 us per layer), while the epilogue reduction (32 lanes x 16 channels x 2 sums per wave through cross-lane moves, behind the
    x shift of the result) lengthens every convolution launch -- same-box A/B of the replayed steps: TaxiBJ 8.13 (pass) / 8.33 (table) /
    10.7 ms (atomics), SST 20.22 / 20.67 / 22.9, Moving-MNIST 7.07 / 7.09."""
    return os.environ.get('VS_BAND_BN_SUMS', '0')


def conv_band_bn_supported(B, Cin, H, W, Cout, groups, dtype):
    """Whether vs_conv3_band (Cin = 4 K plane channels for the k4 s2 family) leaves the BatchNorm sums of its output (band_bn_mode)."""
    if band_bn_mode() == '0' or dtype == torch.float32:
        return False
    return bool(_lib.load_library().vs_conv3_band_bn_supported(code_of(dtype), B, Cin, H, W, Cout, groups))


def conv3_band_parts(x, w_packed, bias, Cout, out_dtype, role='fwd', k4=False):
    """vs_conv3_band / the k4 s2 gather on planes with the per-workgroup (sum, sum of squares) of the stored output written to a table:
    (y, parts [rows, Cout, 2] fp32); bn_stats_from_parts_fold finishes.  No atomics, no zero fill, reproducible."""
    require_cuda(x, w_packed, bias)
    assert x.is_contiguous() and x.dtype == w_packed.dtype
    B, Cin, H, W = x.shape
    lib = _lib.load_library()
    rows = lib.vs_conv3_band_bn_parts_rows(B, H, W)
    assert rows > 0
    y = torch.empty((B, Cout, H, W), dtype=out_dtype, device=x.device)
    parts = torch.empty((rows, Cout, 2), dtype=torch.float32, device=x.device)
    e0 = _pb()
    check(lib.vs_conv3_band_bn_parts(dtype_code(x), x.data_ptr(), w_packed.data_ptr(), _ptr(bias), y.data_ptr(), dtype_code(y), B, Cin, H, W, Cout,
                                     parts.data_ptr(), 1 if k4 else 0, stream_ptr()), 'vs_conv3_band_bn_parts')
    if k4:
        _pe(e0, 'vs_conv_k4s2:%s<%s>' % (role, _DT[dtype_code(x)]), flops=2.0 * B * H * W * Cout * (Cin // 4) * 16,
            nbytes=float(x.numel() * x.element_size() + Cout * (Cin // 4) * 16 * 2 + y.numel() * y.element_size()))
    else:
        _pe(e0, 'vs_conv3_band:%s<%s>' % (role, _DT[dtype_code(x)]), flops=2.0 * B * Cin * H * W * Cout * 9,
            nbytes=float(x.numel() * x.element_size() + w_packed.numel() * 2 + y.numel() * y.element_size()))
    return y, parts


def bn_stats_from_parts_fold(parts, groups, n_per_group, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """(mean, invstd) [groups, C] from the partial-sum table of conv3_band_parts (rows of a call group consecutive) in ONE launch; the running
    estimates are folded in call order."""
    require_cuda(parts)
    rows, C = parts.shape[0], parts.shape[1]
    assert rows % groups == 0
    stats = torch.empty((3, groups, C), dtype=torch.float32, device=parts.device)
    e0 = _pb()
    check(_lib.load_library().vs_bn_stats_from_parts_fold(parts.data_ptr(), rows // groups, groups, C, int(n_per_group), stats[0].data_ptr(),
                                                          stats[1].data_ptr(), stats[2].data_ptr(), _ptr(running_mean), _ptr(running_var),
                                                          float(momentum), float(eps), stream_ptr()), 'vs_bn_stats_from_parts_fold')
    _pe(e0, 'vs_bn_stats_from_sums', nbytes=float(parts.numel() * 4))
    return stats[0], stats[1]


def bn_stats_from_sums_fold(sums, n_per_group, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, reset=True):
    """(mean, invstd) [groups, C] from epilogue sums in ONE launch (running estimates folded in call order; the sums are zeroed for the next step)."""
    require_cuda(sums)
    groups, C = sums.shape[0], sums.shape[1]
    stats = torch.empty((2, groups, C), dtype=torch.float32, device=sums.device)
    e0 = _pb()
    check(_lib.load_library().vs_bn_stats_from_sums_fold(sums.data_ptr(), groups, C, int(n_per_group), stats[0].data_ptr(), stats[1].data_ptr(),
                                                         _ptr(running_mean), _ptr(running_var), float(momentum), float(eps), int(bool(reset)),
                                                         stream_ptr()), 'vs_bn_stats_from_sums_fold')
    _pe(e0, 'vs_bn_stats_from_sums', nbytes=float(sums.numel() * 8))
    return stats[0], stats[1]


def conv3_band(x, w_packed, bias, Cout, out_dtype, role='fwd', bn_sums=None, groups=1):
    """Conv2d k3 s1 p1 of x [B, Cin, H, W] (16-bit) with the `conv3_img16_pack_weight` pre-pack -> y [B, Cout, H, W] in out_dtype (+ bias).
    bn_sums [groups, Cout, 2] (fp64, see bn_sums_buffer): the sums of the stored outputs are added to it in the epilogue."""
    require_cuda(x, w_packed, bias)
    assert x.is_contiguous() and x.dtype == w_packed.dtype
    B, Cin, H, W = x.shape
    y = torch.empty((B, Cout, H, W), dtype=out_dtype, device=x.device)
    e0 = _pb()
    check(_lib.load_library().vs_conv3_band_bn(dtype_code(x), x.data_ptr(), w_packed.data_ptr(), _ptr(bias), y.data_ptr(), dtype_code(y), B, Cin, H, W,
                                               Cout, _ptr(bn_sums), groups, stream_ptr()), 'vs_conv3_band')
    _pe(e0, 'vs_conv3_band:%s<%s>' % (role, _DT[dtype_code(x)]), flops=2.0 * B * Cin * H * W * Cout * 9,
        nbytes=float(x.numel() * x.element_size() + w_packed.numel() * 2 + y.numel() * y.element_size()))
    return y


def slab_sum(slabs, bias, out_dtype, addend=None, addend2=None):
    """sum over the leading (split) axis of fp32 slabs [S, B, C, H, W] (+ bias[c]) (+ addend (+ addend2), fp32 [B, C, H, W]) -> [B, C, H, W] in
    out_dtype, one launch."""
    require_cuda(slabs)
    S, B, C = slabs.shape[0], slabs.shape[1], slabs.shape[2]
    HW = slabs.numel() // (S * B * C)
    if addend is None and addend2 is not None:
        addend, addend2 = addend2, None
    for a in (addend, addend2):
        assert a is None or (a.dtype == torch.float32 and a.is_contiguous() and a.numel() == B * C * HW)
    out = torch.empty(slabs.shape[1:], dtype=out_dtype, device=slabs.device)
    check(_lib.load_library().vs_slab_sum2(slabs.data_ptr(), S, _ptr(bias), _ptr(addend), _ptr(addend2), out.data_ptr(), dtype_code(out), B, C, HW,
                                           stream_ptr()), 'vs_slab_sum')
    return out


def conv_k3_tap_pack_weight(w_master, dtype, flip, out=None):
    """fp32 Conv2d weight [Cout, Cin, 3, 3] -> tap-GEMM rows [ceil(M/28), 9 taps x 28 channels (256 rows), K] in `dtype`.
    flip=False: forward (M = Cout, K = Cin).  flip=True: input gradient (M = Cin, K = Cout, taps flipped)."""
    require_cuda(w_master)
    assert w_master.dtype == torch.float32 and w_master.is_contiguous() and tuple(w_master.shape[2:]) == (3, 3)
    Cout, Cin = w_master.shape[0], w_master.shape[1]
    M, K = (Cin, Cout) if flip else (Cout, Cin)
    lib = _lib.load_library()
    if out is None:
        out = torch.empty((lib.vs_conv_k3_tap_packed_elems(K, M),), dtype=dtype, device=w_master.device)
    check(lib.vs_conv_k3_tap_pack_weight(code_of(dtype), w_master.data_ptr(), K, M, int(bool(flip)), out.data_ptr(), stream_ptr()),
          'vs_conv_k3_tap_pack_weight')
    return out


def conv_k3_tap_fwd(x, w_tap, bias, Cout, out_dtype, groups=1, want_sums=False, role='fwd'):
    """-> (y [B, Cout, H, W] in out_dtype, fp64 sums [groups, Cout, 2] of the stored outputs or None)."""
    require_cuda(x, w_tap, bias)
    assert x.is_contiguous() and x.dtype == w_tap.dtype
    B, Cin, H, W = x.shape
    y = torch.empty((B, Cout, H, W), dtype=out_dtype, device=x.device)
    sums = torch.empty((groups, Cout, 2), dtype=torch.float64, device=x.device) if want_sums else None
    e0 = _pb()
    check(_lib.load_library().vs_conv_k3s1_tap_fwd(dtype_code(x), x.data_ptr(), w_tap.data_ptr(), _ptr(bias), y.data_ptr(), dtype_code(y), _ptr(sums),
                                                   B, Cin, H, W, Cout, groups, stream_ptr()), 'vs_conv_k3s1_tap_fwd')
    _pe(e0, 'vs_conv3_tap:%s<%s>' % (role, _DT[dtype_code(x)]), flops=2.0 * B * Cin * H * W * Cout * 9,
        nbytes=float(x.numel() * x.element_size() + w_tap.numel() * 2 + y.numel() * y.element_size()))
    return y, sums


def bn_stats_from_sums(sums, n_per_group, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """(mean, invstd) [groups, C] from the fp64 (sum, sum of squares) a fused conv epilogue produced; folds the running statistics."""
    require_cuda(sums)
    groups, C = sums.shape[0], sums.shape[1]
    mean = torch.empty((groups, C), dtype=torch.float32, device=sums.device)
    invstd = torch.empty((groups, C), dtype=torch.float32, device=sums.device)
    scratch = torch.empty((groups, C), dtype=torch.float32, device=sums.device) if running_mean is not None else None
    check(_lib.load_library().vs_bn_stats_from_sums(sums.data_ptr(), groups, C, int(n_per_group), mean.data_ptr(), invstd.data_ptr(), _ptr(scratch),
                                                    _ptr(running_mean), _ptr(running_var), float(momentum), float(eps), stream_ptr()),
          'vs_bn_stats_from_sums')
    return mean, invstd


# ------------------------------------------------------------------------------------------------ norm / pool / upsample
def bn_stats(x, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, groups=1):
    """Per-(group, channel) batch statistics; returns (mean [groups, C], invstd [groups, C])."""
    require_cuda(x)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    mean = torch.empty((groups, C), dtype=torch.float32, device=x.device)
    invstd = torch.empty((groups, C), dtype=torch.float32, device=x.device)
    scratch = torch.empty((groups, C), dtype=torch.float32, device=x.device) if running_mean is not None else None
    e0 = _pb()
    check(_lib.load_library().vs_bn_stats(x.data_ptr(), dtype_code(x), B, C, HW, groups, mean.data_ptr(), invstd.data_ptr(),
                                          _ptr(scratch), _ptr(running_mean), _ptr(running_var), float(momentum), float(eps),
                                          stream_ptr()), 'vs_bn_stats')
    _pe(e0, 'vs_bn_stats', nbytes=float(x.numel() * x.element_size()))
    return mean, invstd


def bn_stats_ub(x, eps=1e-5, groups=1):
    """bn_stats without the running update: (mean, invstd, unbiased variance) [groups, C]; `bn_act_fwd(..., running=...)` folds the last one."""
    require_cuda(x)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    stats = torch.empty((3, groups, C), dtype=torch.float32, device=x.device)
    e0 = _pb()
    check(_lib.load_library().vs_bn_stats_ub(x.data_ptr(), dtype_code(x), B, C, HW, groups, stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(),
                                             float(eps), stream_ptr()), 'vs_bn_stats_ub')
    _pe(e0, 'vs_bn_stats', nbytes=float(x.numel() * x.element_size()))
    return stats[0], stats[1], stats[2]


def bn_small_groups_enabled():
    return os.environ.get('VS_BN_SMALL_GROUPS', '0') == '1'


def bn_small_supported(x, groups=1):
    B, C = x.shape[0], x.shape[1]
    if groups > 1:
        # several calls stacked along the batch axis in one launch (vs_bn_train_fwd_small_groups): measured on the TaxiBJ step and NOT the
        # default -- 8.95 ms with it, 8.93 without (the two-launch path's kernels overlap with their neighbours just as well)
        if not bn_small_groups_enabled() or B % groups != 0:
            return False
    # (16-byte vectors: a contiguous slice off 16-byte alignment takes the two-launch forms, as in bn_slab_supported)
    return (x.is_contiguous() and x.data_ptr() % 16 == 0
            and bool(_lib.load_library().vs_bn_train_fwd_small_supported(dtype_code(x), B // groups, C, x.numel() // (B * C))))


def bn_small_supported_shape(dtype, B, C, HW):
    """`bn_small_supported` for a tensor that does not exist yet ([B, C, ...] of HW elements per plane in `dtype`)."""
    return bool(_lib.load_library().vs_bn_train_fwd_small_supported(code_of(dtype), B, C, HW))


def bn_train_fwd_small(x, gamma, beta, act, out_dtype, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, groups=1):
    """Training-mode BatchNorm + activation of one call in ONE launch (small tensors).  Returns (y, mean [1, C], invstd [1, C]).
    groups > 1: that many calls stacked along the batch axis, statistics per call ([groups, C]), running estimates folded in call order."""
    require_cuda(x)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    if groups > 1:
        stats = torch.empty((3, groups, C), dtype=torch.float32, device=x.device)
        e0 = _pb()
        check(_lib.load_library().vs_bn_train_fwd_small_groups(x.data_ptr(), dtype_code(x), y.data_ptr(), dtype_code(y), gamma.data_ptr(), beta.data_ptr(),
                                                               ACT[act], stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(),
                                                               _ptr(running_mean), _ptr(running_var), float(momentum), float(eps), B, C, HW, groups,
                                                               stream_ptr()), 'vs_bn_train_fwd_small_groups')
        _pe(e0, 'vs_bn_fwd_small', nbytes=float(x.numel() * (x.element_size() + y.element_size())))
        return y, stats[0], stats[1]
    mean = torch.empty((1, C), dtype=torch.float32, device=x.device)
    invstd = torch.empty((1, C), dtype=torch.float32, device=x.device)
    e0 = _pb()
    check(_lib.load_library().vs_bn_train_fwd_small(x.data_ptr(), dtype_code(x), y.data_ptr(), dtype_code(y), gamma.data_ptr(), beta.data_ptr(),
                                                    ACT[act], mean.data_ptr(), invstd.data_ptr(), _ptr(running_mean), _ptr(running_var),
                                                    float(momentum), float(eps), B, C, HW, stream_ptr()), 'vs_bn_train_fwd_small')
    _pe(e0, 'vs_bn_fwd_small', nbytes=float(x.numel() * (x.element_size() + y.element_size())))
    return y, mean, invstd


def bn_slab_supported(x, groups=1):
    """A (call group, channel) slab of `x` fits the registers of one workgroup (`bn_train_fwd_slab`: the tensor is read once)."""
    B, C = x.shape[0], x.shape[1]
    return (B % groups == 0 and x.is_contiguous() and x.data_ptr() % 16 == 0
            and bool(_lib.load_library().vs_bn_train_fwd_slab_supported(dtype_code(x), B // groups, C, x.numel() // (B * C))))


def bn_train_fwd_slab(x, gamma, beta, act, out_dtype, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, groups=1):
    """Training-mode BatchNorm + activation of `groups` calls stacked along the batch axis, every (call, channel) slab read ONCE (held in
    registers between the statistics and the apply phase).  Returns (y, mean [groups, C], invstd [groups, C])."""
    require_cuda(x)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    stats = torch.empty((3, groups, C), dtype=torch.float32, device=x.device)
    e0 = _pb()
    check(_lib.load_library().vs_bn_train_fwd_slab(x.data_ptr(), dtype_code(x), y.data_ptr(), dtype_code(y), gamma.data_ptr(), beta.data_ptr(), ACT[act],
                                                   stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(), _ptr(running_mean), _ptr(running_var),
                                                   float(momentum), float(eps), B, C, HW, groups, stream_ptr()), 'vs_bn_train_fwd_slab')
    _pe(e0, 'vs_bn_fwd_slab', nbytes=float(x.numel() * (x.element_size() + y.element_size())))
    return y, stats[0], stats[1]


def bn_train_fwd_small_slabs(slabs, bias, z_dtype, gamma, beta, act, out_dtype, running_mean=None, running_var=None, momentum=0.1, eps=1e-5,
                             skip=None, want16=False):
    """`bn_train_fwd_small` on the split slabs [S, B, C, H, W] (fp32) of `conv3_img16`: the slab sum, the conv bias, the 16-bit rounding of
    the conv output z and the BatchNorm forward in one launch.  Returns (y, z, mean [1, C], invstd [1, C]); with `skip` (fp32, the block
    input of a residual block) additionally (skip + y in fp32, its `z_dtype` copy or None)."""
    require_cuda(slabs)
    S, B, C = slabs.shape[0], slabs.shape[1], slabs.shape[2]
    HW = slabs.numel() // (S * B * C)
    z = torch.empty(slabs.shape[1:], dtype=z_dtype, device=slabs.device)
    y = torch.empty(slabs.shape[1:], dtype=out_dtype, device=slabs.device)
    mean = torch.empty((1, C), dtype=torch.float32, device=slabs.device)
    invstd = torch.empty((1, C), dtype=torch.float32, device=slabs.device)
    xnew = xnew16 = None
    if skip is not None:
        assert skip.dtype == torch.float32 and skip.is_contiguous() and skip.numel() == y.numel()
        xnew = torch.empty(slabs.shape[1:], dtype=torch.float32, device=slabs.device)
        xnew16 = torch.empty(slabs.shape[1:], dtype=z_dtype, device=slabs.device) if want16 else None
    e0 = _pb()
    check(_lib.load_library().vs_bn_train_fwd_small_slabs(slabs.data_ptr(), S, _ptr(bias), z.data_ptr(), dtype_code(z), y.data_ptr(), dtype_code(y),
                                                          gamma.data_ptr(), beta.data_ptr(), ACT[act], mean.data_ptr(), invstd.data_ptr(),
                                                          _ptr(running_mean), _ptr(running_var), float(momentum), float(eps), _ptr(skip),
                                                          _ptr(xnew), _ptr(xnew16), B, C, HW, stream_ptr()), 'vs_bn_train_fwd_small_slabs')
    _pe(e0, 'vs_bn_fwd_small_slabs', nbytes=float(slabs.numel() * 4 + z.numel() * (z.element_size() + y.element_size())))
    if skip is not None:
        return y, z, mean, invstd, xnew, xnew16
    return y, z, mean, invstd


def bn_act_bwd_small_ex(z, mean, invstd, gamma, beta, act, dx_dtype, dy_a=None, dy_b=None, slabs=None, acc=None):
    """One-launch training-mode BatchNorm + activation backward on a small 16-bit z with the upstream gradient from split slabs
    [S, B, C, H, W] or from dy_a (+ dy_b, fp32).  `acc` = (dgamma, dbeta) vectors the parameter gradients are ADDED to (returns
    (dx, None, None)); otherwise fresh (dx, dgamma, dbeta)."""
    require_cuda(z)
    B, C = z.shape[0], z.shape[1]
    HW = z.numel() // (B * C)
    dx = torch.empty(z.shape, dtype=dx_dtype, device=z.device)
    if acc is None:
        dgamma = torch.empty((C,), dtype=torch.float32, device=z.device)
        dbeta = torch.empty((C,), dtype=torch.float32, device=z.device)
    else:
        dgamma, dbeta = acc
        assert dgamma.dtype == torch.float32 and dbeta.dtype == torch.float32 and dgamma.numel() == C and dbeta.numel() == C
    if slabs is not None:
        assert slabs.dtype == torch.float32 and slabs.is_contiguous() and slabs.numel() == slabs.shape[0] * z.numel()
    else:
        assert dy_a is not None and dy_a.is_contiguous() and dy_a.numel() == z.numel()
        assert dy_b is None or (dy_b.dtype == torch.float32 and dy_b.is_contiguous() and dy_b.numel() == z.numel())
    e0 = _pb()
    check(_lib.load_library().vs_bn_act_bwd_small_ex(_ptr(dy_a), dtype_code(dy_a) if dy_a is not None else F32, _ptr(dy_b), _ptr(slabs),
                                                     slabs.shape[0] if slabs is not None else 0, z.data_ptr(), dtype_code(z), mean.data_ptr(),
                                                     invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ACT[act], dgamma.data_ptr(),
                                                     dbeta.data_ptr(), int(acc is not None), dx.data_ptr(), dtype_code(dx), B, C, HW, stream_ptr()),
          'vs_bn_act_bwd_small_ex')
    _pe(e0, 'vs_bn_bwd_small_ex', nbytes=float(z.numel() * (z.element_size() + dx.element_size() + 4)))
    if acc is not None:
        return dx, None, None
    return dx, dgamma, dbeta


# ---- a ConvResBlock layer in one launch (csrc/vs_conv_img.hip: conv3_img16_bn_kernel) -------------------------------------------------
_IMGBN = {}          # device index -> {'ws': int32 workspace (word 0: epoch base, word 1: sticky error flag), 'idx': launches since the last advance}


def _imgbn_state(device):
    """The exchange workspace of the fused layers on `device` (one per device: the integrator's launches follow each other on one stream).
    Created OUTSIDE a stream capture (GraphedStep's warm-up steps reach it first): a workspace created while capturing would be zero-filled
    and re-initialised by every replay."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    st = _IMGBN.get(index)
    if st is None:
        exchange_guard(device)
        nbytes = _lib.load_library().vs_conv3_img16_bn_workspace_bytes()
        ws = torch.zeros((nbytes // 4,), dtype=torch.int32, device=device)
        ws[0] = 65536                                    # epochs start above zero: a zero-filled granule never looks current
        st = _IMGBN[index] = {'ws': ws, 'idx': 0}
    return st


def _imgbn_next_call(st):
    st['idx'] += 1
    if st['idx'] >= 65535:                               # (a step has ~1000 such launches; callers outside a training step never advance)
        check(_lib.load_library().vs_exchange_epoch_advance(st['ws'].data_ptr(), stream_ptr()), 'vs_exchange_epoch_advance')
        st['idx'] = 1
    return st['idx']


def exchange_epoch_advance(device=None):
    """Start of a training step: the launch numbers of the fused layers restart at 1 under a new epoch base (one 1-thread launch, recordable:
    a replayed step then tags its exchanges with epochs no earlier replay used).  No-op while no fused layer has run on the device."""
    index = torch.cuda.current_device() if device is None or device.index is None else device.index
    st = _IMGBN.get(index)
    if st is None:
        return
    check(_lib.load_library().vs_exchange_epoch_advance(st['ws'].data_ptr(), stream_ptr()), 'vs_exchange_epoch_advance')
    st['idx'] = 0


def conv3_img16_bn_supported(B, Cin, Cout, dtype, act='leaky_relu', out_dtype=None, backward=False):
    """Whether conv3_img16_bn_fwd / _bwd serve a Conv2d k3 s1 p1 (Cin -> Cout) -> BatchNorm -> `act` layer on B maps of 16 x 16 with output type
    `out_dtype` (forward).  VS_IMG_BN_SPLITS (default '1'): the input-channel split counts served -- with several
    splits the partial sums cross the chip inside the launch, which costs what the kernel boundary it replaces costs (measured)."""
    if dtype == torch.float32:
        return False
    lib = _lib.load_library()
    if not lib.vs_conv3_img16_bn_supported(code_of(dtype), B, Cin, Cout):
        return False
    if not lib.vs_conv3_img16_bn_form_supported(int(backward), ACT[act], code_of(out_dtype if out_dtype is not None else dtype), code_of(dtype)):
        return False
    allowed = os.environ.get('VS_IMG_BN_SPLITS', '1').split(',')
    return str(lib.vs_conv3_img16_splits(B, Cin, Cout)) in allowed


def conv3_img16_bn_fwd(x, w_packed, bias, gamma, beta, act, out_dtype, Cout, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, skip=None,
                       want16=False):
    """act(BatchNorm_train(conv3x3(x) + bias)) of ONE call in ONE launch: (y, z, mean [1, C], invstd [1, C]) like conv3_img16 +
    bn_train_fwd_small_slabs; with `skip` additionally (skip + y in fp32, its 16-bit copy or None)."""
    require_cuda(x, w_packed)
    assert x.is_contiguous() and x.dtype == w_packed.dtype and tuple(x.shape[2:]) == (16, 16)
    B, Cin = x.shape[0], x.shape[1]
    st = _imgbn_state(x.device)
    z = torch.empty((B, Cout, 16, 16), dtype=x.dtype, device=x.device)
    y = torch.empty((B, Cout, 16, 16), dtype=out_dtype, device=x.device)
    mean = torch.empty((1, Cout), dtype=torch.float32, device=x.device)
    invstd = torch.empty((1, Cout), dtype=torch.float32, device=x.device)
    xnew = xnew16 = None
    if skip is not None:
        assert skip.dtype == torch.float32 and skip.is_contiguous() and skip.numel() == y.numel()
        xnew = torch.empty((B, Cout, 16, 16), dtype=torch.float32, device=x.device)
        xnew16 = torch.empty((B, Cout, 16, 16), dtype=x.dtype, device=x.device) if want16 else None
    e0 = _pb()
    check(_lib.load_library().vs_conv3_img16_bn_fwd(dtype_code(x), x.data_ptr(), w_packed.data_ptr(), st['ws'].data_ptr(), _imgbn_next_call(st), _ptr(bias),
                                                    gamma.data_ptr(), beta.data_ptr(), ACT[act], _ptr(running_mean), _ptr(running_var), float(momentum),
                                                    float(eps), z.data_ptr(), y.data_ptr(), dtype_code(y), mean.data_ptr(), invstd.data_ptr(), _ptr(skip),
                                                    _ptr(xnew), _ptr(xnew16), B, Cin, Cout, stream_ptr()), 'vs_conv3_img16_bn_fwd')
    _pe(e0, 'vs_conv3_img16_bn:fwd<%s>' % _DT[dtype_code(x)], flops=2.0 * B * 256 * Cout * Cin * 9,
        nbytes=float(x.numel() * x.element_size() + w_packed.numel() * 2 + z.numel() * (z.element_size() + y.element_size())))
    if skip is not None:
        return y, z, mean, invstd, xnew, xnew16
    return y, z, mean, invstd


def conv3_img16_bn_bwd(dz_next, w_packed_flipped, Cout, z, mean, invstd, gamma, beta, act, acc=None):
    """The backward layer in ONE launch: dz = BatchNorm + activation backward (from the stored z, mean, invstd) of dy = the input gradient of the
    FOLLOWING layer's convolution of dz_next (`w_packed_flipped`: that layer's weight, flip = 1).  `acc` = (dgamma, dbeta) the parameter
    gradients are ADDED to (returns (dz, None, None)); otherwise fresh (dz, dgamma, dbeta)."""
    require_cuda(dz_next, w_packed_flipped, z)
    assert dz_next.is_contiguous() and z.is_contiguous() and dz_next.dtype == z.dtype == w_packed_flipped.dtype
    B, Cin = dz_next.shape[0], dz_next.shape[1]
    assert z.shape[0] == B and z.shape[1] == Cout
    st = _imgbn_state(z.device)
    dz = torch.empty(z.shape, dtype=z.dtype, device=z.device)
    if acc is None:
        dgamma = torch.empty((Cout,), dtype=torch.float32, device=z.device)
        dbeta = torch.empty((Cout,), dtype=torch.float32, device=z.device)
    else:
        dgamma, dbeta = acc
        assert dgamma.dtype == torch.float32 and dbeta.dtype == torch.float32 and dgamma.numel() == Cout and dbeta.numel() == Cout
    e0 = _pb()
    check(_lib.load_library().vs_conv3_img16_bn_bwd(dtype_code(z), dz_next.data_ptr(), w_packed_flipped.data_ptr(), st['ws'].data_ptr(), _imgbn_next_call(st),
                                                    z.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ACT[act],
                                                    dz.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), int(acc is not None), B, Cin, Cout, stream_ptr()),
          'vs_conv3_img16_bn_bwd')
    _pe(e0, 'vs_conv3_img16_bn:bwd<%s>' % _DT[dtype_code(z)], flops=2.0 * B * 256 * Cout * Cin * 9,
        nbytes=float(dz_next.numel() * 2 + w_packed_flipped.numel() * 2 + 2 * z.numel() * z.element_size()))
    if acc is not None:
        return dz, None, None
    return dz, dgamma, dbeta


def bn_act_fwd(x, mean, invstd, gamma, beta, act, out_dtype, groups=1, running=None):
    """y = act(gamma * (x - mean) * invstd + beta) per (call group, channel).  running = (ubvar [groups, C], running_mean, running_var, momentum):
    the running estimates are folded in call order by the same launch (bn_stats_ub produced ubvar)."""
    require_cuda(x)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    e0 = _pb()
    if running is not None:
        ub, rm, rv, momentum = running
        check(_lib.load_library().vs_bn_act_fwd_running(x.data_ptr(), dtype_code(x), y.data_ptr(), dtype_code(y), mean.data_ptr(), invstd.data_ptr(),
                                                        gamma.data_ptr(), beta.data_ptr(), ACT[act], B, C, HW, groups, ub.data_ptr(), rm.data_ptr(),
                                                        rv.data_ptr(), float(momentum), stream_ptr()), 'vs_bn_act_fwd_running')
    else:
        check(_lib.load_library().vs_bn_act_fwd(x.data_ptr(), dtype_code(x), y.data_ptr(), dtype_code(y), mean.data_ptr(),
                                                invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ACT[act], B, C, HW, groups,
                                                stream_ptr()), 'vs_bn_act_fwd')
    _pe(e0, 'vs_bn_act_fwd', nbytes=float(x.numel() * (x.element_size() + y.element_size())))
    return y


def bn_act_bwd(dy, x, mean, invstd, gamma, beta, act, training, out_dtype, groups=1):
    """Returns (dx, dgamma [C], dbeta [C]) -- the per-call-group sums are added up by the kernel itself (vs_bn_act_bwd_gsum)."""
    require_cuda(dy, x)
    dy = dy.contiguous()
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    per_group = torch.empty((2, groups, C), dtype=torch.float32, device=x.device)
    dgamma, dbeta = per_group[0], per_group[1]
    sums = torch.empty((2, C), dtype=torch.float32, device=x.device) if groups > 1 else None
    dx = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    e0 = _pb()
    check(_lib.load_library().vs_bn_act_bwd_gsum(dy.data_ptr(), dtype_code(dy), x.data_ptr(), dtype_code(x), mean.data_ptr(),
                                                 invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ACT[act], int(bool(training)),
                                                 groups, dgamma.data_ptr(), dbeta.data_ptr(), dx.data_ptr(), dtype_code(dx), B, C, HW,
                                                 _ptr(sums[0]) if sums is not None else 0, _ptr(sums[1]) if sums is not None else 0,
                                                 stream_ptr()), 'vs_bn_act_bwd')
    _pe(e0, 'vs_bn_act_bwd', nbytes=float(x.numel() * (2 * x.element_size() + 2 * dy.element_size() + dx.element_size())))
    if groups == 1:
        return dx, dgamma[0], dbeta[0]
    return dx, sums[0], sums[1]


def chan_sum(x):
    require_cuda(x)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    out = torch.empty((C,), dtype=torch.float32, device=x.device)
    lib = _lib.load_library()
    ws = _workspace(lib.vs_chan_sum_workspace_bytes(B, C, HW), x.device)
    e0 = _pb()
    check(lib.vs_chan_sum_ws(x.data_ptr(), dtype_code(x), B, C, HW, ws.data_ptr(), ws.numel(), out.data_ptr(), stream_ptr()), 'vs_chan_sum_ws')
    _pe(e0, 'vs_chan_sum<%s>' % _DT[dtype_code(x)], nbytes=float(x.numel() * x.element_size()))
    return out


def maxpool2_fwd(x):
    require_cuda(x)
    B, C, H, W = x.shape
    y = torch.empty((B, C, H // 2, W // 2), dtype=x.dtype, device=x.device)
    check(_lib.load_library().vs_maxpool2_fwd(x.data_ptr(), dtype_code(x), y.data_ptr(), dtype_code(y), B * C, H, W, stream_ptr()),
          'vs_maxpool2_fwd')
    return y


def maxpool2_bwd(x, dy):
    require_cuda(x, dy)
    B, C, H, W = x.shape
    dy = dy.contiguous()
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    check(_lib.load_library().vs_maxpool2_bwd(x.data_ptr(), dtype_code(x), dy.data_ptr(), dtype_code(dy), dx.data_ptr(),
                                              dtype_code(dx), B * C, H, W, stream_ptr()), 'vs_maxpool2_bwd')
    return dx


def maxpool3s2_fwd(x):
    """nn.MaxPool2d(3, 2, 1) on [B, C, H, W]."""
    require_cuda(x)
    B, C, H, W = x.shape
    y = torch.empty((B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=x.dtype, device=x.device)
    check(_lib.load_library().vs_maxpool3s2_fwd(x.data_ptr(), dtype_code(x), y.data_ptr(), dtype_code(y), B * C, H, W, stream_ptr()),
          'vs_maxpool3s2_fwd')
    return y


def maxpool3s2_bwd(x, dy):
    require_cuda(x, dy)
    B, C, H, W = x.shape
    dy = dy.contiguous()
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    check(_lib.load_library().vs_maxpool3s2_bwd(x.data_ptr(), dtype_code(x), dy.data_ptr(), dtype_code(dy), dx.data_ptr(),
                                                dtype_code(dx), B * C, H, W, stream_ptr()), 'vs_maxpool3s2_bwd')
    return dx


def upsample2_fwd(x):
    require_cuda(x)
    B, C, H, W = x.shape
    y = torch.empty((B, C, 2 * H, 2 * W), dtype=x.dtype, device=x.device)
    check(_lib.load_library().vs_upsample2_fwd(x.data_ptr(), dtype_code(x), y.data_ptr(), dtype_code(y), B * C, H, W, stream_ptr()),
          'vs_upsample2_fwd')
    return y


def upsample2_bwd(dy, out_dtype):
    require_cuda(dy)
    dy = dy.contiguous()
    B, C, H2, W2 = dy.shape
    dx = torch.empty((B, C, H2 // 2, W2 // 2), dtype=out_dtype, device=dy.device)
    check(_lib.load_library().vs_upsample2_bwd(dy.data_ptr(), dtype_code(dy), dx.data_ptr(), dtype_code(dx), B * C, H2 // 2, W2 // 2,
                                               stream_ptr()), 'vs_upsample2_bwd')
    return dx


# ------------------------------------------------------------------------------------------------ fused frame losses
def frames_sse_fwd(frames, full, idx):
    """frames [B, G, D] fp32, full [B, T, D] fp32, idx [G] int32 (device) -> sums [2] (frame 0; frames 1..)."""
    require_cuda(frames, full, idx)
    assert frames.is_contiguous() and full.is_contiguous() and frames.dtype == torch.float32 and full.dtype == torch.float32
    B, G, D = frames.shape
    sums = torch.empty((2,), dtype=torch.float32, device=frames.device)
    e0 = _pb()
    check(_lib.load_library().vs_frames_sse_fwd(frames.data_ptr(), full.data_ptr(), idx.data_ptr(), B, G, full.shape[1], D,
                                                sums.data_ptr(), stream_ptr()), 'vs_frames_sse_fwd')
    _pe(e0, 'vs_frames_sse_fwd', nbytes=float(2 * frames.numel() * 4))
    return sums


def _loss_args(frames, full, idx, s_old, s_new, t0, lambdas, average_tloss):
    import ctypes
    if isinstance(idx, tuple):                       # (t_random int32 [1] on the device, ae_shift, first_forecast)
        t_dev, ae_shift, first_forecast = idx
        assert t_dev.dtype == torch.int32 and t_dev.numel() == 1
        require_cuda(t_dev)
        idx_args = (None, t_dev.data_ptr(), int(ae_shift), int(first_forecast))
    else:
        require_cuda(idx)
        assert idx.dtype == torch.int32 and idx.is_contiguous()
        idx_args = (idx.data_ptr(), None, 0, 0)
    require_cuda(frames, full, t0)
    assert frames.is_contiguous() and full.is_contiguous() and t0.is_contiguous()
    assert frames.dtype == torch.float32 and full.dtype == torch.float32 and t0.dtype == torch.float32
    B, G, D = frames.shape
    n_s = 0 if s_old is None else s_old.numel()
    if n_s:
        require_cuda(s_old, s_new)
        assert s_old.is_contiguous() and s_new.is_contiguous() and s_old.dtype == torch.float32 and s_new.dtype == torch.float32
    lam = (ctypes.c_float * 4)(*[float(v) for v in lambdas])
    return (frames.data_ptr(), full.data_ptr()) + idx_args + (B, G, full.shape[1], D, _ptr(s_old) if n_s else None,
            _ptr(s_new) if n_s else None, n_s, t0.data_ptr(), t0.shape[0], t0.numel() // t0.shape[0], int(bool(average_tloss)),
            ctypes.cast(lam, ctypes.c_void_p)), lam


def train_losses_fwd(frames, full, idx, s_old, s_new, t0, lambdas, average_tloss):
    """-> out [10] device floats: [4] total, [5] ae, [6] zero-order, [7] pred, [8] t_reg.  lambdas = (ae, s, t, pred)."""
    args, keep = _loss_args(frames, full, idx, s_old, s_new, t0, lambdas, average_tloss)
    out = torch.empty((10,), dtype=torch.float32, device=frames.device)
    e0 = _pb()
    check(_lib.load_library().vs_train_losses_fwd(*args, out.data_ptr(), stream_ptr()), 'vs_train_losses_fwd')
    _pe(e0, 'vs_train_losses_fwd', nbytes=float(2 * frames.numel() * 4))
    return out


def train_losses_fwd_grad(frames, full, idx, s_old, s_new, t0, lambdas, average_tloss, grad_total, frames_act, dz_dtype):
    """train_losses_fwd and train_losses_bwd (dz form) in one pass, for the upstream gradient `grad_total` (one device float) known now.
    -> (out [10], dz, ds_old, ds_new, dt0)."""
    args, keep = _loss_args(frames, full, idx, s_old, s_new, t0, lambdas, average_tloss)
    require_cuda(grad_total)
    assert grad_total.dtype == torch.float32 and grad_total.numel() == 1
    out = torch.empty((16 + 2 * 4096,), dtype=torch.float32, device=frames.device)      # [0..9] results, [16..] per-workgroup partial sums
    dz = torch.empty(frames.shape, dtype=dz_dtype, device=frames.device)
    ds_old = torch.empty_like(s_old) if s_old is not None else None
    ds_new = torch.empty_like(s_new) if s_new is not None else None
    dt0 = torch.empty_like(t0)
    e0 = _pb()
    check(_lib.load_library().vs_train_losses_fwd_grad(*args, out.data_ptr(), grad_total.data_ptr(), _ptr(ds_old), _ptr(ds_new), dt0.data_ptr(),
                                                       ACT[frames_act], dz.data_ptr(), dtype_code(dz), stream_ptr()), 'vs_train_losses_fwd_grad')
    _pe(e0, 'vs_train_losses_fwd', nbytes=float(2 * frames.numel() * 4 + dz.numel() * dz.element_size()))
    return out, dz, ds_old, ds_new, dt0


def gemm_frame_loss(h, w, bias, act, full, idx, G, s_old, s_new, t0, lambdas, average_tloss, grad_total, dz_dtype):
    """The decoder's last layer with the frame losses in its epilogue (vs_gemm_frame_loss): h [B * G, K] and w [N, K] 16-bit, the frames
    act(h w^T + bias) are compared with full [B, T, N] in registers and never stored.  idx = (t_random int32 [1] on the device, ae_shift,
    first_forecast).  -> (out, dz [B * G, N], ds_old, ds_new, dt0) as train_losses_fwd_grad, or None when the problem does not run on the
    256 x 256 tile kernel (the caller then stores the frames and uses train_losses_fwd_grad)."""
    import ctypes
    require_cuda(h, w, bias, full, s_old, s_new, t0, grad_total)
    t_dev, ae_shift, first_forecast = idx
    require_cuda(t_dev)
    assert h.dtype == w.dtype and h.dtype in (torch.bfloat16, torch.float16) and h.stride(-1) == 1 and w.stride(-1) == 1
    assert full.dtype == torch.float32 and full.is_contiguous() and full.dim() == 3 and t0.is_contiguous() and t0.dtype == torch.float32
    assert t_dev.dtype == torch.int32 and t_dev.numel() == 1 and grad_total.dtype == torch.float32 and grad_total.numel() == 1
    M, K = h.shape
    N = w.shape[0]
    assert M % G == 0 and full.shape[0] == M // G and full.shape[2] == N
    n_s = 0 if s_old is None else s_old.numel()
    lam = (ctypes.c_float * 4)(*[float(v) for v in lambdas])
    out = torch.empty((16 + 2 * 4096,), dtype=torch.float32, device=h.device)
    dz = torch.empty((M, N), dtype=dz_dtype, device=h.device)
    ds_old = torch.empty_like(s_old) if n_s else None
    ds_new = torch.empty_like(s_new) if n_s else None
    dt0 = torch.empty_like(t0)
    e0 = _pb()
    rc = _lib.load_library().vs_gemm_frame_loss(
        dtype_code(h), M, N, K, h.data_ptr(), h.stride(0), w.data_ptr(), w.stride(0), _ptr(bias), ACT[act], full.data_ptr(), t_dev.data_ptr(),
        int(ae_shift), int(first_forecast), int(G), full.shape[1], _ptr(s_old) if n_s else None, _ptr(s_new) if n_s else None, n_s, t0.data_ptr(),
        t0.shape[0], t0.numel() // t0.shape[0], int(bool(average_tloss)), ctypes.cast(lam, ctypes.c_void_p), grad_total.data_ptr(), dz.data_ptr(),
        dtype_code(dz), _ptr(ds_old), _ptr(ds_new), dt0.data_ptr(), out.data_ptr(), stream_ptr())
    if rc == -4:                                     # VS_ERR_UNSUPPORTED
        return None
    check(rc, 'vs_gemm_frame_loss')
    _pe(e0, 'vs_gemm<%s,RR>' % _DT[dtype_code(h)], flops=2.0 * M * N * K,
        nbytes=float((M * K + N * K) * h.element_size() + M * N * (4 + dz.element_size())))
    return out, dz, ds_old, ds_new, dt0


def train_losses_bwd(frames, full, idx, s_old, s_new, t0, lambdas, average_tloss, grad_total, frames_act=None, dz_dtype=None):
    """-> (dframes, ds_old, ds_new, dt0).  With `frames_act` (the activation whose outputs `frames` are) the first result is instead
    the gradient of that activation's input, dframes * act'(frames), in `dz_dtype`."""
    args, keep = _loss_args(frames, full, idx, s_old, s_new, t0, lambdas, average_tloss)
    require_cuda(grad_total)
    fused = frames_act is not None
    dframes = torch.empty(frames.shape, dtype=dz_dtype if fused else torch.float32, device=frames.device)
    ds_old = torch.empty_like(s_old) if s_old is not None else None
    ds_new = torch.empty_like(s_new) if s_new is not None else None
    dt0 = torch.empty_like(t0)
    e0 = _pb()
    check(_lib.load_library().vs_train_losses_bwd(*args, grad_total.data_ptr(), None if fused else dframes.data_ptr(), _ptr(ds_old),
                                                  _ptr(ds_new), dt0.data_ptr(), ACT[frames_act] if fused else 0,
                                                  dframes.data_ptr() if fused else None, dtype_code(dframes) if fused else 0, stream_ptr()),
          'vs_train_losses_bwd')
    _pe(e0, 'vs_train_losses_bwd', nbytes=float(2 * frames.numel() * 4 + dframes.numel() * dframes.element_size()))
    return dframes, ds_old, ds_new, dt0


def gather_windows(data, item_idx, windows_per_seq, seq_len, pixel_idx=None, out_dtype=torch.float32):
    """data [n_seq, nt, frame] fp32 on the device, item_idx int32 [B] -> [B, seq_len, frame (or len(pixel_idx))]."""
    require_cuda(data, item_idx, pixel_idx)
    assert data.dtype == torch.float32 and data.is_contiguous() and data.dim() == 3
    assert item_idx.dtype == torch.int32 and item_idx.is_contiguous()
    n_seq, nt, frame = data.shape
    B = item_idx.numel()
    n_pix = 0
    if pixel_idx is not None:
        assert pixel_idx.dtype == torch.int32 and pixel_idx.is_contiguous()
        n_pix = pixel_idx.numel()
    out = torch.empty((B, seq_len, n_pix if pixel_idx is not None else frame), dtype=out_dtype, device=data.device)
    e0 = _pb()
    check(_lib.load_library().vs_gather_windows(data.data_ptr(), n_seq, nt, frame, item_idx.data_ptr(), B, int(windows_per_seq), int(seq_len),
                                                _ptr(pixel_idx), n_pix, out.data_ptr(), dtype_code(out), stream_ptr()), 'vs_gather_windows')
    _pe(e0, 'vs_gather_windows', nbytes=float(out.numel() * (4 + out.element_size())))
    return out


def wave_source_table(f0, T, dt):
    """(source fp32 [n_seq, 3 (T - 1) + 1], h fp32 [T - 1]) on the host: the reference's source f0 * exp(-20 t) (gen_wave.py:27-28, 124) at the
    stage times of torchdiffeq's fixed-grid rk4, rounded as the reference rounds it.  The grid is arange(0, dt * T, dt) in fp32 (computed
    in double, rounded per element); the stage times t0, t0 + h / 3, t0 + 2 h / 3 are formed in fp32, widened by `.item()`, and the source
    is evaluated in fp64 and rounded when it meets the fp32 mask; the last entry is the fourth stage of the last step, t[T - 1].  The
    grid comes from the reference's own call (gen_wave.py:134), on the host: torch rounds its points in a way no closed form restates.
    Where dt * T / dt rounds up past T the call yields T + 1 points; the first T are used."""
    import numpy as np
    t = torch.arange(0, float(dt) * T, float(dt), dtype=torch.float32, device='cpu')[:T].numpy()
    assert t.size == T
    h = t[1:] - t[:-1]
    stages = np.stack([t[:-1], t[:-1] + h * np.float32(1.0 / 3.0), t[:-1] + h * np.float32(2.0 / 3.0)], axis=1).reshape(-1)
    times = np.concatenate([stages, t[-1:]]).astype(np.float64)
    f0 = np.asarray(f0, dtype=np.float64).reshape(-1, 1)
    return (f0 * np.exp(-20.0 * times)[None, :]).astype(np.float32), h


def wave_simulate(f0, c, T, dt=0.001, init=None, normalise=False, device=None):
    """The reference's WaveEq simulations (preprocessing/wave/gen_wave.py) for the source amplitudes `f0` and velocities `c` (sequences of
    floats), `T` frames `dt` apart, in ONE launch of vs_wave_simulate -> (simul fp32 [n_seq, T, 64, 64], minmax fp32 [n_seq, 2]) on the
    device.  init: optional fp32 [n_seq, 2, 64, 64] device tensor, the initial (w, w'); None = zeros like the reference.  normalise=True
    returns every sequence as (x - min) / (max - min); minmax always holds the raw extremes.  Only the parameter tables cross PCIe."""
    import numpy as np
    f0 = np.asarray(f0, dtype=np.float64).reshape(-1)
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    n_seq, T = f0.size, int(T)
    if n_seq < 1 or c.size != n_seq or T < 1:
        raise _lib.VarsepHipError('wave_simulate needs one (f0, c) pair per sequence and T >= 1 (got %d, %d, T = %d)' % (f0.size, c.size, T))
    device = torch.device(device if device is not None else (init.device if init is not None else 'cuda'))
    if device.type != 'cuda':
        raise _lib.VarsepHipError('wave_simulate runs on an MI355X device; there is no CPU fallback (tests use tests/wave_sim_ref.py)')
    if init is not None:
        require_cuda(init)
        assert init.dtype == torch.float32 and init.is_contiguous() and tuple(init.shape) == (n_seq, 2, 64, 64) and init.device == device
    source, h = wave_source_table(f0, T, dt)
    c2 = (c * c).astype(np.float32)                                 # gen_wave.py:85: the Python float c**2 meets an fp32 tensor
    table = torch.from_numpy(np.concatenate([c2, h, source.reshape(-1)])).to(device)
    c2_d, h_d, source_d = table[:n_seq], table[n_seq:n_seq + T - 1], table[n_seq + T - 1:]
    with torch.cuda.device(device):
        simul = torch.empty((n_seq, T, 64, 64), dtype=torch.float32, device=device)
        minmax = torch.empty((n_seq, 2), dtype=torch.float32, device=device)
        e0 = _pb()
        check(_lib.load_library().vs_wave_simulate(n_seq, T, 64, c2_d.data_ptr(), source_d.data_ptr(), h_d.data_ptr() if T > 1 else None,
                                                   _ptr(init), simul.data_ptr(), minmax.data_ptr(), int(bool(normalise)), stream_ptr()),
              'vs_wave_simulate')
        _pe(e0, 'vs_wave_simulate', flops=float(n_seq) * (T - 1) * 4 * 4096 * 30, nbytes=float(simul.numel() * 4 * (3 if normalise else 1)))
    return simul, minmax


def lanczos_coeffs(in_size, out_size):
    """(k int32 [out_size, ksize], bounds int32 [out_size, 2] = (first tap, taps)) of PIL's 8-bit Lanczos resampling of an axis of `in_size`
    pixels to `out_size` (ImagingResample: `precompute_coeffs` + `normalize_coeffs_8bpc`, 22 fractional bits), on the host.  Python floats
    (C doubles) and math.sin throughout: NumPy's vectorised sine may differ by an ulp, which can flip a rounded coefficient.  Entries of
    a row beyond its taps are 0.  Checked once per table: every |k| < 2^23 (the kernel's 24-bit multiply is exact) and
    255 * max row sum|k| + 2^21 < 2^31 (its 32-bit accumulator cannot overflow)."""
    import math
    import numpy as np
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise _lib.VarsepHipError('lanczos_coeffs: sizes must be positive (got %d -> %d)' % (in_size, out_size))

    def sinc(x):
        if x == 0.0:
            return 1.0
        x = x * math.pi
        return math.sin(x) / x

    def lanczos(x):
        return sinc(x) * sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0

    in0, in1 = 0.0, float(in_size)
    scale = (in1 - in0) / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    k = np.zeros((out_size, ksize), dtype=np.int64)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [lanczos((x + xmin - center + 0.5) / fs) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k[xx, :xmax] = [int(v * 4194304.0 + 0.5) if v >= 0 else int(v * 4194304.0 - 0.5) for v in w]
        bounds[xx] = (xmin, xmax)
    if int(np.abs(k).max()) >= 1 << 23 or 255 * int(np.abs(k).sum(axis=1).max()) + (1 << 21) >= 1 << 31:
        raise _lib.VarsepHipError('lanczos_coeffs(%d, %d): a coefficient needs more than 24 bits or a row sum overflows 32 bits' % (in_size, out_size))
    return k.astype(np.int32), bounds


_resample_tables = {}


def _lanczos_tables(extent, size, device):
    """(k, bounds) of an axis on `device`, built once per (extent, size, device)."""
    key = (int(extent), int(size), device.type, device.index)
    if key not in _resample_tables:
        k, b = lanczos_coeffs(extent, size)
        _resample_tables[key] = (torch.from_numpy(k).to(device), torch.from_numpy(b).to(device), k.shape[1])
    return _resample_tables[key]


def resample_lanczos_u8(images_u8, box, size):
    """uint8 [n, H, W, C] on the device -> uint8 [n, size_h, size_w, C]: `Image.fromarray(img).crop(box).resize(size, Image.LANCZOS)` of every
    image, bit for bit, in ONE launch of vs_resample_u8 (csrc/vs_resample.hip).  box = (left, upper, right, lower) as PIL orders it;
    size = (w, h), or an int for a square output; C in 1..4.  The coefficient tables are cached on the device per (extent, size, device)."""
    require_cuda(images_u8)
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4:
        raise _lib.VarsepHipError('resample_lanczos_u8: uint8 [n, H, W, C] expected (got %s %s)' % (images_u8.dtype, tuple(images_u8.shape)))
    out_w, out_h = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    left, upper, right, lower = (int(v) for v in box)
    n, H, W, C = images_u8.shape
    if not (0 <= left < right <= W and 0 <= upper < lower <= H) or out_w < 1 or out_h < 1 or n < 1:
        raise _lib.VarsepHipError('resample_lanczos_u8: box %s must lie inside the %d x %d images, and the batch and the output size %s be '
                                  'positive' % ((left, upper, right, lower), W, H, (out_w, out_h)))
    images_u8 = images_u8.contiguous()
    device = images_u8.device
    with torch.cuda.device(device):
        kx, bx, ksx = _lanczos_tables(right - left, out_w, device)
        ky, by, ksy = _lanczos_tables(lower - upper, out_h, device)
        out = torch.empty((n, out_h, out_w, C), dtype=torch.uint8, device=device)
        e0 = _pb()
        check(_lib.load_library().vs_resample_u8(images_u8.data_ptr(), n, H, W, C, left, upper, right - left, lower - upper, kx.data_ptr(),
                                                 bx.data_ptr(), ksx, ky.data_ptr(), by.data_ptr(), ksy, out_w, out_h, out.data_ptr(),
                                                 stream_ptr()), 'vs_resample_u8')
        _pe(e0, 'vs_resample_u8', flops=2.0 * n * C * (float(lower - upper) * out_w * ksx + float(out_h) * out_w * ksy),
            nbytes=float(n) * C * ((lower - upper) * (right - left) + out_h * out_w))
    return out


# ---- PNG decoding on the device (csrc/vs_png.hip) ----------------------------------------------------------------------------------
INFLATE_STATUS = {1: 'bad zlib header', 2: 'reserved block type', 3: 'stored-block length mismatch',
                  4: 'bad, over-subscribed or incomplete code lengths', 5: 'invalid symbol or distance code',
                  6: 'distance before the start of the output', 7: 'compressed data ends early', 8: 'more image data than the header announces',
                  9: 'less image data than the header announces', 10: 'Adler-32 mismatch', 11: 'unknown PNG filter type'}


def inflate_zlib(packed, offsets, out_len, out_stride):
    """`n` zlib streams in one launch of vs_inflate_zlib.  packed: uint8 [bytes] on the device, the streams back to back (any alignment);
    offsets: int64 [n + 1]; out_len: int64 [n], the exact length every stream must produce.  Returns (out uint8 [n, out_stride], status
    int32 [n], produced int64 [n]); stream i is out[i, :out_len[i]] when status[i] == 0 (INFLATE_STATUS names the other values), and a
    damaged stream fails alone.  Bytes of a slot beyond what its stream produced are not written."""
    require_cuda(packed, offsets, out_len)
    if packed.dtype != torch.uint8 or packed.dim() != 1 or offsets.dtype != torch.int64 or offsets.dim() != 1 or out_len.dtype != torch.int64 \
            or out_len.dim() != 1 or offsets.numel() != out_len.numel() + 1 or out_len.numel() < 1 or int(out_stride) < 1:
        raise _lib.VarsepHipError('inflate_zlib: packed uint8 [bytes], offsets int64 [n + 1], out_len int64 [n], n >= 1 and out_stride >= 1 '
                                  'expected')
    if not packed.is_contiguous():
        packed = packed.contiguous()
    offsets, out_len = offsets.contiguous(), out_len.contiguous()
    n, device = out_len.numel(), packed.device
    with torch.cuda.device(device):
        out = torch.empty((n, int(out_stride)), dtype=torch.uint8, device=device)
        status = torch.empty((n,), dtype=torch.int32, device=device)
        produced = torch.empty((n,), dtype=torch.int64, device=device)
        e0 = _pb()
        check(_lib.load_library().vs_inflate_zlib(packed.data_ptr(), packed.numel(), offsets.data_ptr(), n, out_len.data_ptr(), out.data_ptr(),
                                                  int(out_stride), status.data_ptr(), produced.data_ptr(), stream_ptr()), 'vs_inflate_zlib')
        _pe(e0, 'vs_inflate_zlib', nbytes=float(packed.numel()) + float(n) * int(out_stride))
    return out, status, produced


def png_unfilter(raw, status, H, W, C):
    """raw: uint8 [n, stride >= H * (1 + W * C)] on the device, the filtered rows of n images (what inflate_zlib returns); status int32 [n]
    of the inflate launch -> pixels uint8 [n, H, W, C], all five PNG filter types undone in one launch of vs_png_unfilter.  An image whose
    status is not 0 is skipped; a filter byte above 4 sets its status to 11 (in place)."""
    require_cuda(raw, status)
    if raw.dtype != torch.uint8 or raw.dim() != 2 or raw.stride(1) != 1 or status.dtype != torch.int32 or status.dim() != 1 \
            or not status.is_contiguous() or status.numel() != raw.shape[0]:
        raise _lib.VarsepHipError('png_unfilter: raw uint8 [n, stride] with contiguous rows and status int32 [n] expected')
    n, device = raw.shape[0], raw.device
    with torch.cuda.device(device):
        pixels = torch.empty((n, int(H), int(W), int(C)), dtype=torch.uint8, device=device)
        e0 = _pb()
        check(_lib.load_library().vs_png_unfilter(raw.data_ptr(), raw.stride(0), n, int(H), int(W), int(C), pixels.data_ptr(), status.data_ptr(),
                                                  stream_ptr()), 'vs_png_unfilter')
        _pe(e0, 'vs_png_unfilter', nbytes=float(n) * int(H) * (1 + 2 * int(W) * int(C)))
    return pixels


def png_pack(blobs, names=None):
    """The host part of png_decode_rgb8: every file's chunks are parsed as data/chairs.py's `read_png_rgb8` parses them (signature, IHDR,
    concatenated IDAT bodies, stop at IEND) and the zlib streams are packed back to back.  Returns (W, H, packed uint8 array, offsets int64
    [n + 1]).  ValueError naming the file for a damaged file or one of another size than the first; `chairs.PngNotCovered` (a ValueError)
    for a file the kernels do not decode (no PNG signature, or not 8-bit non-interlaced RGB)."""
    import numpy as np
    from .data import chairs
    names = ['image %d of the batch' % i for i in range(len(blobs))] if names is None else list(names)
    if not blobs or len(names) != len(blobs):
        raise ValueError('png_pack: a non-empty batch and one name per file are expected')
    streams, size = [], None
    for blob, name in zip(blobs, names):
        (width, height, depth, colour, _, _, interlace), idat = chairs.png_chunks(blob, name)
        if (depth, colour, interlace) != (8, 2, 0):
            raise chairs.PngNotCovered('%s: an 8-bit non-interlaced RGB PNG is expected (bit depth %d, colour type %d, interlace %d)'
                                       % (name, depth, colour, interlace))
        if width < 1 or height < 1:
            raise ValueError('%s: a PNG of %d x %d pixels' % (name, width, height))
        if size is None:
            size = (width, height)
        elif (width, height) != size:
            raise ValueError('%s: a %d x %d image among %d x %d ones (a batch is one tensor)' % (name, width, height, size[0], size[1]))
        streams.append(b''.join(idat))
    offsets = np.zeros(len(streams) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in streams], out=offsets[1:])
    packed = np.frombuffer(bytearray(b''.join(streams) or b'\0'), dtype=np.uint8)      # (writable: torch shares it)
    return size[0], size[1], packed, offsets


def png_decode_packed(packed, offsets, H, W, C=3):
    """The device part: packed uint8 [bytes] and offsets int64 [n + 1] on the device -> (pixels uint8 [n, H, W, C], status int32 [n]); the
    two launches."""
    n = offsets.numel() - 1
    size = H * (1 + W * C)
    out_len = torch.full((n,), size, dtype=torch.int64, device=packed.device)
    raw, status, _ = inflate_zlib(packed, offsets, out_len, size)
    return png_unfilter(raw, status, H, W, C), status


def png_status_error(status, names=None):
    """The ValueError for the first non-zero entry of a status tensor (naming the file and the reason), or None.  Reads the statuses back."""
    bad = status.cpu().numpy()
    for i in bad.nonzero()[0]:
        name = names[i] if names is not None else 'image %d of the batch' % i
        return ValueError('%s: %s (decoder status %d)' % (name, INFLATE_STATUS.get(int(bad[i]), 'unknown status'), int(bad[i])))
    return None


def png_decode_rgb8(blobs, names=None, device=None, check_status=False):
    """blobs: the bytes of n non-interlaced 8-bit RGB PNG files of one common size -> (uint8 [n, H, W, 3] on the device, status int32 [n]):
    the chunks are parsed and the compressed streams packed on the host, only the COMPRESSED bytes are uploaded, and two launches decode
    them (inflate, then the row filters).  Pixels of image i are valid where status[i] == 0; check_status=True reads the statuses back
    and raises ValueError naming the first failed file and the reason."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    W, H, packed, offsets = png_pack(blobs, names)
    pixels, status = png_decode_packed(torch.from_numpy(packed).to(device), torch.from_numpy(offsets).to(device), H, W, 3)
    if check_status:
        err = png_status_error(status, names)
        if err is not None:
            raise err
    return pixels, status


def chairs_gather(frames_u8, desc, seq_len, out_dtype=torch.float32, validate=True):
    """frames_u8 uint8 [n_objects, views, H, W, C] on the device, desc int32 [rows, 2] = (object, first view) -> [rows, seq_len, C, H, W]
    in `out_dtype`: frame t of a row is view (first + t) % views, values byte / 255 (vs_chairs_gather, one launch).
    validate=True reads back the launch's error word (a host sync) and raises VarsepHipError for a descriptor out of range;
    validate=False keeps the call free of host syncs (the caller has checked the table)."""
    require_cuda(frames_u8, desc)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 5 or desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != 2:
        raise _lib.VarsepHipError('chairs_gather: frames uint8 [n_objects, views, H, W, C] and desc int32 [rows, 2] expected')
    frames_u8, desc = frames_u8.contiguous(), desc.contiguous()
    n, views, H, W, C = frames_u8.shape
    rows = desc.shape[0]
    out = torch.empty((rows, max(int(seq_len), 0), C, H, W), dtype=out_dtype, device=frames_u8.device)
    bad = torch.zeros((1,), dtype=torch.int32, device=frames_u8.device) if validate else None
    e0 = _pb()
    check(_lib.load_library().vs_chairs_gather(frames_u8.data_ptr(), n, views, H, W, C, desc.data_ptr(), rows, int(seq_len), out.data_ptr(),
                                               _lib.code_of(out_dtype), _ptr(bad), stream_ptr()), 'vs_chairs_gather')
    _pe(e0, 'vs_chairs_gather', nbytes=float(out.numel() * (1 + out.element_size())))
    if validate and int(bad.item()):
        raise _lib.VarsepHipError('chairs_gather: a descriptor names an object outside [0, %d) or a first view outside [0, %d)' % (n, views))
    return out


def gather_timeline(frames, first, item_idx, seq_len, step, out_dtype=torch.float32, validate=True):
    """frames fp32 [n_frames, frame_elems] on the device, first int32 [n_windows] (frame at position 0 of every window), item_idx int32
    [rows] -> [rows, seq_len, frame_elems] in `out_dtype`: out[r, k] = frames[first[item_idx[r]] + k * step], step +1 or -1
    (vs_gather_timeline, one launch).  validate=True reads back the launch's error word (a host sync) and raises VarsepHipError for an
    item outside the table or a window that leaves the timeline; validate=False keeps the call free of host syncs."""
    require_cuda(frames, first, item_idx)
    if (frames.dtype != torch.float32 or frames.dim() != 2 or first.dtype != torch.int32 or first.dim() != 1
            or item_idx.dtype != torch.int32 or item_idx.dim() != 1):
        raise _lib.VarsepHipError('gather_timeline: frames fp32 [n_frames, frame_elems], first int32 [n_windows] and item_idx int32 [rows] expected')
    frames, first, item_idx = frames.contiguous(), first.contiguous(), item_idx.contiguous()
    n_frames, frame = frames.shape
    rows = item_idx.numel()
    out = torch.empty((rows, max(int(seq_len), 0), frame), dtype=out_dtype, device=frames.device)
    bad = torch.zeros((1,), dtype=torch.int32, device=frames.device) if validate else None
    e0 = _pb()
    check(_lib.load_library().vs_gather_timeline(frames.data_ptr(), n_frames, frame, first.data_ptr(), first.numel(), int(step), item_idx.data_ptr(),
                                                 rows, int(seq_len), out.data_ptr(), _lib.code_of(out_dtype), _ptr(bad), stream_ptr()),
          'vs_gather_timeline')
    _pe(e0, 'vs_gather_timeline', nbytes=float(out.numel() * (4 + out.element_size())))
    if validate and int(bad.item()):
        raise _lib.VarsepHipError('gather_timeline: an item index is outside [0, %d) or a window leaves the %d frames of the timeline'
                                  % (first.numel(), n_frames))
    return out


_MIXING = {'concat': 0, 'mul': 1}


def mix_codes_fwd(s, t_rand, t_codes, mixing, lowp=None):
    """-> (z [B, 1+n, Cz] fp32, the same in the 16-bit dtype `lowp` or None); mixing 'concat' | 'mul' (mlp_encdec.py:43-48)."""
    require_cuda(s, t_rand, t_codes)
    assert s.dtype == t_rand.dtype == t_codes.dtype == torch.float32
    assert s.is_contiguous() and t_rand.is_contiguous() and t_codes.is_contiguous()
    B, Cs = s.shape
    n, Ct = t_codes.shape[1], t_codes.shape[2]
    assert t_rand.shape == (B, Ct) and t_codes.shape[0] == B
    Cz = Cs if mixing == 'mul' else Cs + Ct
    z = torch.empty((B, n + 1, Cz), dtype=torch.float32, device=s.device)
    z_lowp = torch.empty((B, n + 1, Cz), dtype=lowp, device=s.device) if lowp is not None else None
    e0 = _pb()
    check(_lib.load_library().vs_mix_codes_fwd(s.data_ptr(), t_rand.data_ptr(), t_codes.data_ptr(), B, n, Cs, Ct, _MIXING[mixing],
                                               z.data_ptr(), _ptr(z_lowp), code_of(lowp) if lowp is not None else BF16, stream_ptr()), 'vs_mix_codes_fwd')
    _pe(e0, 'vs_mix_codes_fwd', nbytes=float(z.numel() * 8))
    return z, z_lowp


def mix_codes_bwd(dz, s, t_rand, t_codes, mixing):
    require_cuda(dz, s, t_rand, t_codes)
    assert dz.dtype == torch.float32 and dz.is_contiguous()
    B, Cs = s.shape
    n, Ct = t_codes.shape[1], t_codes.shape[2]
    ds, dt_rand, dt_codes = torch.empty_like(s), torch.empty_like(t_rand), torch.empty_like(t_codes)
    e0 = _pb()
    check(_lib.load_library().vs_mix_codes_bwd(dz.data_ptr(), s.data_ptr(), t_rand.data_ptr(), t_codes.data_ptr(), B, n, Cs, Ct,
                                               _MIXING[mixing], ds.data_ptr(), dt_rand.data_ptr(), dt_codes.data_ptr(), stream_ptr()),
          'vs_mix_codes_bwd')
    _pe(e0, 'vs_mix_codes_bwd', nbytes=float(dz.numel() * 8))
    return ds, dt_rand, dt_codes


def frames_sse_bwd(frames, full, idx, coef):
    require_cuda(frames, full, idx, coef)
    B, G, D = frames.shape
    out = torch.empty_like(frames)
    e0 = _pb()
    check(_lib.load_library().vs_frames_sse_bwd(frames.data_ptr(), full.data_ptr(), idx.data_ptr(), B, G, full.shape[1], D,
                                                coef.data_ptr(), out.data_ptr(), stream_ptr()), 'vs_frames_sse_bwd')
    _pe(e0, 'vs_frames_sse_bwd', nbytes=float(3 * frames.numel() * 4))
    return out


def cat_bcast_supported(a, x, n):
    return (a.is_cuda and x.is_cuda and a.dim() == 4 and x.dim() == 4 and a.is_contiguous() and x.is_contiguous() and x.shape[0] == n * a.shape[0]
            and a.shape[2:] == x.shape[2:] and (a.shape[2] * a.shape[3]) % 8 == 0 and a.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
            and a.dtype in (torch.float32, torch.bfloat16, torch.float16) and x.dtype in (torch.float32, torch.bfloat16, torch.float16))


def cat_bcast_fwd(a, x, n, out_dtype):
    """cat([a.repeat(n, 1, 1, 1), x], dim=1) in out_dtype: a [B, Ca, H, W], x [n B, Cb, H, W] -> [n B, Ca + Cb, H, W], one pass."""
    require_cuda(a, x)
    B, Ca = a.shape[0], a.shape[1]
    Cb, HW = x.shape[1], x.shape[2] * x.shape[3]
    out = torch.empty((n * B, Ca + Cb) + tuple(x.shape[2:]), dtype=out_dtype, device=x.device)
    e0 = _pb()
    check(_lib.load_library().vs_cat_bcast_fwd(a.data_ptr(), dtype_code(a), x.data_ptr(), dtype_code(x), out.data_ptr(), dtype_code(out), B, n, Ca, Cb, HW,
                                               stream_ptr()), 'vs_cat_bcast_fwd')
    _pe(e0, 'vs_cat_bcast', nbytes=float(x.numel() * x.element_size() + out.numel() * out.element_size()))
    return out


def cat_bcast_bwd(dout, B, n, Ca, a_dtype, x_dtype, need_a=True, need_x=True):
    """(da [B, Ca, H, W] = sum over the n frames of dout[:, :Ca], dx [n B, Cb, H, W] = dout[:, Ca:]) in one pass over dout."""
    require_cuda(dout)
    dout = dout.contiguous()
    C, H, W = dout.shape[1], dout.shape[2], dout.shape[3]
    Cb = C - Ca
    da = torch.empty((B, Ca, H, W), dtype=a_dtype, device=dout.device) if need_a else None
    dx = torch.empty((n * B, Cb, H, W), dtype=x_dtype, device=dout.device) if need_x else None
    e0 = _pb()
    check(_lib.load_library().vs_cat_bcast_bwd(dout.data_ptr(), dtype_code(dout), _ptr(da), code_of(a_dtype), _ptr(dx), code_of(x_dtype), B, n, Ca, Cb, H * W,
                                               stream_ptr()), 'vs_cat_bcast_bwd')
    _pe(e0, 'vs_cat_bcast', nbytes=float(dout.numel() * dout.element_size() * 2))
    return da, dx


def _code_loss_tables(pairs):
    import ctypes
    n = len(pairs)
    VP, I32, I64 = ctypes.c_void_p * max(n, 1), ctypes.c_int32 * max(n, 1), ctypes.c_int64 * max(n, 1)
    return n, VP, I32(*([dtype_code(a) for a, _ in pairs] or [0])), I64(*([a.numel() for a, _ in pairs] or [0]))


def code_losses_supported(pairs, t0):
    """Whether the fused code-loss kernels take these (a, b) pairs: <= 10 of them, equal shapes / types, contiguous, element counts multiples of 8."""
    if len(pairs) > 10 or t0 is None or t0.dtype != torch.float32 or not t0.is_contiguous() or not t0.is_cuda:
        return False
    for a, b in pairs:
        if (a.shape != b.shape or a.dtype != b.dtype or not a.is_cuda or not a.is_contiguous() or not b.is_contiguous() or a.numel() % 8 != 0
                or a.numel() == 0 or a.dtype not in (torch.float32, torch.bfloat16, torch.float16) or a.data_ptr() % 16 or b.data_ptr() % 16):
            return False
    return True


def code_losses_fwd(pairs, t0, sse_ae, sse_pred, scale_ae, scale_pred, lambdas, inv_t):
    """out [5] = (total, ae, zero, pred, t_reg) from the pairs of the zero-order loss, the initial temporal code and the raw frame sums
    (vs_code_losses_fwd: a partial-sum launch over 4096-element chunks + a one-block finish)."""
    require_cuda(t0, sse_ae, sse_pred)
    lib = _lib.load_library()
    n, VP, dts, cnts = _code_loss_tables(pairs)
    total = sum(a.numel() for a, _ in pairs)
    chunks = lib.vs_code_losses_chunks(n, cnts, t0.numel())
    partial = torch.empty((max(int(chunks), 1),), dtype=torch.float32, device=t0.device)
    out = torch.empty((5,), dtype=torch.float32, device=t0.device)
    l_ae, l_s, l_t, l_pred = (float(v) for v in lambdas)
    e0 = _pb()
    check(lib.vs_code_losses_fwd(n, VP(*([a.data_ptr() for a, _ in pairs] or [0])), VP(*([b.data_ptr() for _, b in pairs] or [0])), dts, cnts, t0.data_ptr(),
                                 t0.numel(), sse_ae.data_ptr(), sse_pred.data_ptr(), float(scale_ae), float(scale_pred), l_ae, l_s, l_pred, l_t,
                                 1.0 / max(total, 1), float(inv_t), partial.data_ptr(), out.data_ptr(), stream_ptr()), 'vs_code_losses_fwd')
    _pe(e0, 'vs_code_losses_fwd', nbytes=float(sum(2 * a.numel() * a.element_size() for a, _ in pairs) + t0.numel() * 4))
    return out


def code_losses_bwd(pairs, need, t0, g, scale_ae, scale_pred, lambdas, inv_t):
    """(d a_j or None, d b_j or None per pair, d t0, coefs [4]) for the upstream gradient g (one fp32 element on the device); need[j] = (bool, bool)."""
    require_cuda(t0, g)
    lib = _lib.load_library()
    n, VP, dts, cnts = _code_loss_tables(pairs)
    total = sum(a.numel() for a, _ in pairs)
    da = [torch.empty_like(a) if need[j][0] else None for j, (a, _) in enumerate(pairs)]
    db = [torch.empty_like(b) if need[j][1] else None for j, (_, b) in enumerate(pairs)]
    dt0 = torch.empty_like(t0)
    coefs = torch.empty((4,), dtype=torch.float32, device=t0.device)
    l_ae, l_s, l_t, l_pred = (float(v) for v in lambdas)
    e0 = _pb()
    check(lib.vs_code_losses_bwd(n, VP(*([a.data_ptr() for a, _ in pairs] or [0])), VP(*([b.data_ptr() for _, b in pairs] or [0])),
                                 VP(*([_ptr(t) for t in da] or [0])), VP(*([_ptr(t) for t in db] or [0])), dts, cnts, t0.data_ptr(), dt0.data_ptr(), t0.numel(),
                                 g.data_ptr(), float(scale_ae), float(scale_pred), l_ae, l_s, l_pred, l_t, 1.0 / max(total, 1), float(inv_t), coefs.data_ptr(),
                                 stream_ptr()), 'vs_code_losses_bwd')
    _pe(e0, 'vs_code_losses_bwd', nbytes=float(sum(4 * a.numel() * a.element_size() for a, _ in pairs) + t0.numel() * 8))
    return da, db, dt0, coefs


# ------------------------------------------------------------------------------------------------ fp16 loss scaling
def check_finite_multi(grads, scale_state):
    """scale_state[1] (found_inf) = 1 when any gradient tensor holds an inf / NaN; one launch per 64 tensors."""
    import ctypes
    require_cuda(scale_state, *grads)
    assert scale_state.dtype == torch.float32 and scale_state.numel() >= 4
    lib = _lib.load_library()
    found = scale_state.data_ptr() + 4
    for i in range(0, len(grads), 64):
        chunk = grads[i:i + 64]
        n = len(chunk)
        for g in chunk:
            assert g.is_contiguous()
        VP, I32, I64 = ctypes.c_void_p * n, ctypes.c_int32 * n, ctypes.c_int64 * n
        e0 = _pb()
        check(lib.vs_check_finite_multi(n, VP(*[g.data_ptr() for g in chunk]), I32(*[dtype_code(g) for g in chunk]),
                                        I64(*[g.numel() for g in chunk]), found, stream_ptr()), 'vs_check_finite_multi')
        _pe(e0, 'vs_check_finite_multi', nbytes=float(sum(g.numel() * g.element_size() for g in chunk)))


def loss_scale_update(scale_state, growth_factor, backoff_factor, growth_interval):
    require_cuda(scale_state)
    check(_lib.load_library().vs_loss_scale_update(scale_state.data_ptr(), float(growth_factor), float(backoff_factor), int(growth_interval),
                                                   stream_ptr()), 'vs_loss_scale_update')


# ------------------------------------------------------------------------------------------------ evaluation metrics
def frame_metrics(pred, target, max_val=1.0, k1=0.01, k2=0.03, sigma=1.5, want_ssim=True):
    """pred, target [..., H, W] fp32 (any leading dims): per-plane (mse, mean SSIM) with the leading shape (vs_frame_metrics)."""
    require_cuda(pred, target)
    assert pred.shape == target.shape and pred.dim() >= 2
    H, W = pred.shape[-2], pred.shape[-1]
    lead = tuple(pred.shape[:-2])
    p = pred.reshape(-1, H, W).float().contiguous()
    t = target.reshape(-1, H, W).float().contiguous()
    mse = torch.empty((p.shape[0],), dtype=torch.float32, device=p.device)
    ssim = torch.empty((p.shape[0],), dtype=torch.float32, device=p.device) if want_ssim else None
    check(_lib.load_library().vs_frame_metrics(p.data_ptr(), t.data_ptr(), p.shape[0], H, W, float(max_val), float(k1), float(k2), float(sigma),
                                               mse.data_ptr(), _ptr(ssim), stream_ptr()), 'vs_frame_metrics')
    return mse.view(lead), (ssim.view(lead) if want_ssim else None)


def frame_metrics_multi(pred, targets, max_val=1.0, k1=0.01, k2=0.03, sigma=1.5, want_mse=True, want_ssim=True):
    """pred [B, ..., H, W] fp32 against targets [B, P, ..., H, W] fp32: per-plane (mse, mean SSIM) of shape [B, P, ...]
    (vs_frame_metrics_multi; vs_frame_metrics against each of the P targets, with the prediction staged once)."""
    require_cuda(pred, targets)
    if targets.dim() != pred.dim() + 1 or targets.shape[0] != pred.shape[0] or targets.shape[2:] != pred.shape[1:] or pred.dim() < 3:
        raise _lib.VarsepHipError('frame_metrics_multi: targets must be [B, P] + pred.shape[1:] (got %s and %s)'
                                  % (tuple(pred.shape), tuple(targets.shape)))
    B, P, H, W = pred.shape[0], targets.shape[1], pred.shape[-2], pred.shape[-1]
    lead = tuple(pred.shape[1:-2])
    per = 1
    for d in lead:
        per *= d
    p = pred.float().contiguous()
    t = targets.float().contiguous()
    mse = torch.empty((B, P) + lead, dtype=torch.float32, device=p.device) if want_mse else None
    ssim = torch.empty((B, P) + lead, dtype=torch.float32, device=p.device) if want_ssim else None
    check(_lib.load_library().vs_frame_metrics_multi(p.data_ptr(), t.data_ptr(), B, P, per, H, W, float(max_val), float(k1), float(k2), float(sigma),
                                                     _ptr(mse), _ptr(ssim), stream_ptr()), 'vs_frame_metrics_multi')
    return mse, ssim


def sst_frame_metrics(pred, target, consts, day0, zone, zone_range, k1=0.01, k2=0.03, sigma=1.5, validate=True):
    """The metrics of the SST evaluation script (test/sst/test.py:57-71) in one launch (vs_sst_frame_metrics).  pred, target fp32
    [rows, T, H, W]: normalised forecasts and targets; consts fp32 [n_days, 4] = (mu_norm, std_norm, mu_clim, std_clim); day0, zone int32
    [rows]: day of the first target frame, position in zone_range fp32 [n_zones, 2] = (min, max) -> (mse [rows, T], ssim [rows, T, T]),
    where ssim[r, t, c] pairs frame t with the constants of day day0 + c.  validate=True reads back the launch's error word (a host sync)
    and raises VarsepHipError for a row whose days leave `consts` or whose zone is out of range (such a row is written as zeros);
    validate=False keeps the call free of host syncs."""
    require_cuda(pred, target, consts, day0, zone, zone_range)
    if (pred.dtype != torch.float32 or target.dtype != torch.float32 or pred.dim() != 4 or pred.shape != target.shape
            or consts.dtype != torch.float32 or consts.dim() != 2 or consts.shape[1] != 4
            or zone_range.dtype != torch.float32 or zone_range.dim() != 2 or zone_range.shape[1] != 2
            or day0.dtype != torch.int32 or zone.dtype != torch.int32 or day0.shape != (pred.shape[0],) or zone.shape != (pred.shape[0],)):
        raise _lib.VarsepHipError('sst_frame_metrics: pred / target fp32 [rows, T, H, W], consts fp32 [n_days, 4], day0 / zone int32 [rows] and '
                                  'zone_range fp32 [n_zones, 2] expected')
    pred, target, consts, day0, zone, zone_range = (x.contiguous() for x in (pred, target, consts, day0, zone, zone_range))
    rows, T, H, W = pred.shape
    mse = torch.empty((rows, T), dtype=torch.float32, device=pred.device)
    ssim = torch.empty((rows, T, T), dtype=torch.float32, device=pred.device)
    bad = torch.zeros((1,), dtype=torch.int32, device=pred.device) if validate else None
    check(_lib.load_library().vs_sst_frame_metrics(pred.data_ptr(), target.data_ptr(), rows, T, H, W, consts.data_ptr(), consts.shape[0],
                                                   day0.data_ptr(), zone.data_ptr(), zone_range.data_ptr(), zone_range.shape[0], float(k1),
                                                   float(k2), float(sigma), mse.data_ptr(), ssim.data_ptr(), _ptr(bad), stream_ptr()),
          'vs_sst_frame_metrics')
    if validate and int(bad.item()):
        raise _lib.VarsepHipError('sst_frame_metrics: a row names days outside the %d of `consts` or a zone outside [0, %d)'
                                  % (consts.shape[0], zone_range.shape[0]))
    return mse, ssim


def moving_mnist_batch(digits, init, seq_len, frame_size, out_dtype=torch.float32):
    """Training videos [B, seq_len, 1, F, F] with values in [0, 1] from the draws `init` int32 [B, nd, 5] = (digit index, start row, start
    column, row speed, column speed) in ONE launch (vs_moving_mnist_batch).  digits uint8 [N, h, w]; both on the device, nothing is read
    back.  A digit index outside [0, N) draws nothing."""
    require_cuda(digits, init)
    if digits.dtype != torch.uint8 or digits.dim() != 3 or init.dtype != torch.int32 or init.dim() != 3 or init.shape[2] != 5:
        raise _lib.VarsepHipError('moving_mnist_batch: digits uint8 [N, h, w] and init int32 [B, nd, 5] expected')
    digits, init = digits.contiguous(), init.contiguous()
    out = torch.empty((init.shape[0], seq_len, 1, frame_size, frame_size), dtype=out_dtype, device=digits.device)
    check(_lib.load_library().vs_moving_mnist_batch(digits.data_ptr(), digits.shape[0], digits.shape[1], digits.shape[2], init.data_ptr(),
                                                    init.shape[0], init.shape[1], seq_len, frame_size, out.data_ptr(), dtype_code(out),
                                                    stream_ptr()), 'vs_moving_mnist_batch')
    return out


def moving_mnist_place(digits, positions, desc, seq_len, frame_size, out_dtype=torch.float32, validate=True):
    """Videos [V, seq_len, 1, F, F] with the digits `desc[v, 1 + i]` at `positions[t, desc[v, 0], i]` (vs_moving_mnist_place).
    digits uint8 [N, h, w], positions int32 [T >= seq_len, n_seq, nd, 2], desc int32 [V, 1 + nd], all on the device.
    validate=True reads back the launch's error word (a host sync) and raises VarsepHipError for an index out of range or a digit that
    would be cut at the frame border; validate=False keeps the call free of host syncs (the caller has checked the table)."""
    require_cuda(digits, positions, desc)
    if digits.dtype != torch.uint8 or digits.dim() != 3 or positions.dtype != torch.int32 or positions.dim() != 4 or positions.shape[3] != 2 \
            or desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != 1 + positions.shape[2] or positions.shape[0] < seq_len:
        raise _lib.VarsepHipError('moving_mnist_place: digits uint8 [N, h, w], positions int32 [T >= seq_len, n_seq, nd, 2], '
                                  'desc int32 [V, 1 + nd] expected')
    digits, positions, desc = digits.contiguous(), positions.contiguous(), desc.contiguous()
    V, nd = desc.shape[0], positions.shape[2]
    out = torch.empty((V, seq_len, 1, frame_size, frame_size), dtype=out_dtype, device=digits.device)
    bad = torch.zeros((1,), dtype=torch.int32, device=digits.device) if validate else None
    check(_lib.load_library().vs_moving_mnist_place(digits.data_ptr(), digits.shape[0], digits.shape[1], digits.shape[2], positions.data_ptr(),
                                                    positions.shape[1], nd, desc.data_ptr(), V, seq_len, frame_size, out.data_ptr(),
                                                    dtype_code(out), _ptr(bad), stream_ptr()), 'vs_moving_mnist_place')
    if validate and int(bad.item()):
        raise _lib.VarsepHipError('moving_mnist_place: a sequence / digit index is out of range or a digit does not lie inside the '
                                  '%d x %d frame' % (frame_size, frame_size))
    return out


def moving_mnist_testset(digits, init, seq_len, frame_size, *, fp32=False, time_major=True):
    """The Moving-MNIST test videos and their latents in ONE launch (vs_moving_mnist_testset).  digits uint8 [N, h, w] on the device; init
    int32 [V, nd, 5] = (digit index, start row, start column, row speed, column speed), a host array or a tensor -> (frames, latents):
    frames hold the raw values 0..255, uint8 or (fp32=True) float32, shaped [seq_len, V, 1, F, F] (time_major, the test file's layout) or
    [V, seq_len, 1, F, F]; latents int32 [seq_len, V, nd, 4] = (row, column, row speed, column speed) per frame.  `init` is checked on the
    host (a device tensor is read back: a host sync): a digit index outside [0, N) or a start position outside the frame raises, and so does a
    non-zero speed along an axis on which the digit fills the frame (no room: the reference's bounce loop never ends there)."""
    import numpy as np
    require_cuda(digits)
    host = init.detach().cpu().numpy() if isinstance(init, torch.Tensor) else np.asarray(init)
    if digits.dtype != torch.uint8 or digits.dim() != 3 or host.dtype != np.int32 or host.ndim != 3 or host.shape[2] != 5 or host.shape[0] < 1 \
            or int(seq_len) < 1:
        raise _lib.VarsepHipError('moving_mnist_testset: digits uint8 [N, h, w], init int32 [V >= 1, nd, 5] and seq_len >= 1 expected')
    N, h, w = digits.shape
    V, nd = host.shape[0], host.shape[1]
    seq_len, F = int(seq_len), int(frame_size)
    if host[..., 0].min() < 0 or host[..., 0].max() >= N or host[..., 1:3].min() < 0 or host[..., 1].max() > F - h or host[..., 2].max() > F - w:
        raise _lib.VarsepHipError('moving_mnist_testset: init names a digit outside [0, %d) or a start position outside the %d x %d frame'
                                  % (N, F, F))
    if (F == h and host[..., 3].any()) or (F == w and host[..., 4].any()):
        # the reference's bounce loop never ends here (each pass mirrors the position about the single allowed point); the kernel's loop
        # is bounded at 64 passes and would leave an arbitrary position
        raise _lib.VarsepHipError('moving_mnist_testset: a %d x %d digit has no room to move in a %d x %d frame, yet init gives one a speed '
                                  'along that axis (the reference does not terminate on this)' % (h, w, F, F))
    digits = digits.contiguous()
    device = digits.device
    dev_init = init.to(device).contiguous() if isinstance(init, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(host)).to(device)
    with torch.cuda.device(device):
        return _mmnist_testset_launch('vs_moving_mnist_testset', seq_len, V, F, fp32, time_major, device, seq_len * V * nd * 16,
                                      lambda: torch.empty((seq_len, V, nd, 4), dtype=torch.int32, device=device),
                                      lambda *out: (digits.data_ptr(), N, h, w, dev_init.data_ptr(), V, nd, seq_len, F, *out, stream_ptr()))


def _mmnist_testset_launch(entry, T, V, F, fp32, time_major, device, other_bytes, second, args):
    """What the two test-set renderers do alike -> (frames, second output): the raw frames, uint8 or (fp32) float32, [T, V, 1, F, F]
    (time_major) or [V, T, 1, F, F]; then second() (the latents / the error word or None); then the entry point `entry` with args(frames
    pointer, fp32 flag, stride of t, stride of v, pointer of the second output).  other_bytes: what the launch moves beside the frames."""
    frames = torch.empty((T, V, 1, F, F) if time_major else (V, T, 1, F, F), dtype=torch.float32 if fp32 else torch.uint8, device=device)
    other = second()
    stride_t, stride_v = (frames.stride(0), frames.stride(1)) if time_major else (frames.stride(1), frames.stride(0))
    e0 = _pb()
    check(getattr(_lib.load_library(), entry)(*args(frames.data_ptr(), 1 if fp32 else 0, stride_t, stride_v, _ptr(other))), entry)
    _pe(e0, entry, nbytes=float(frames.numel() * frames.element_size() + other_bytes))
    return frames, other


def moving_mnist_testset_place(digits, positions, digit_idx, frame_size, *, fp32=False, time_major=True, validate=True):
    """The RAW test-set frames of `moving_mnist_testset` from STORED positions, in ONE launch (vs_moving_mnist_testset_place): the renderer
    of the stochastic test set, whose trajectories mmnist_stochastic_trajectories walks.  digits uint8 [N, h, w], positions int32 [T, V, nd,
    2] = (row, column) of the top-left corners, digit_idx int32 [V, nd], all on the device -> frames with the raw values 0..255, uint8 or
    (fp32=True) float32, shaped [T, V, 1, F, F] (time_major, the test file's layout) or [V, T, 1, F, F].  validate=True reads back the
    launch's error word (a host sync) and raises VarsepHipError for a digit index outside [0, N) or a digit that would be cut at the frame
    border (such a digit is not drawn); validate=False keeps the call free of host syncs (the caller has checked the tables)."""
    require_cuda(digits, positions, digit_idx)
    if digits.dtype != torch.uint8 or digits.dim() != 3 or positions.dtype != torch.int32 or positions.dim() != 4 or positions.shape[3] != 2 \
            or positions.shape[0] < 1 or positions.shape[1] < 1 or digit_idx.dtype != torch.int32 or digit_idx.dim() != 2 \
            or tuple(digit_idx.shape) != tuple(positions.shape[1:3]):
        raise _lib.VarsepHipError('moving_mnist_testset_place: digits uint8 [N, h, w], positions int32 [T >= 1, V >= 1, nd, 2] and digit_idx '
                                  'int32 [V, nd] expected')
    digits, positions, digit_idx = digits.contiguous(), positions.contiguous(), digit_idx.contiguous()
    N, h, w = digits.shape
    T, V, nd = positions.shape[:3]
    F = int(frame_size)
    device = digits.device
    with torch.cuda.device(device):
        frames, bad = _mmnist_testset_launch(
            'vs_moving_mnist_testset_place', T, V, F, fp32, time_major, device, positions.numel() * 4,
            lambda: torch.zeros((1,), dtype=torch.int32, device=device) if validate else None,
            lambda *out: (digits.data_ptr(), N, h, w, positions.data_ptr(), digit_idx.data_ptr(), V, nd, T, F, *out, stream_ptr()))
    if validate and int(bad.item()):
        raise _lib.VarsepHipError('moving_mnist_testset_place: a digit index is outside [0, %d) or a digit does not lie inside the %d x %d frame'
                                  % (N, F, F))
    return frames


def frames_to_u8_nhwc(x, out=None):
    """[B, T, C, H, W] fp32 / 16-bit -> uint8 [B, T, H, W, C] on the device: (uint8)(x * 255.f), i.e. `x.mul(255).byte().permute(0, 1, 3, 4, 2)`
    bit for bit for x in [0, 1]; out-of-range values saturate to 0 / 255 (NaN -> 0) where torch's cast is undefined (vs_frames_to_u8_nhwc).
    out: optional contiguous uint8 [B, T, H, W, C] tensor on x's device, written in place and returned (a slice of a preallocated
    [N, T, H, W, C] buffer, for instance); anything else is refused."""
    require_cuda(x, out)
    if x.dim() != 5:
        raise _lib.VarsepHipError('frames_to_u8_nhwc: [B, T, C, H, W] expected (got %s)' % (tuple(x.shape),))
    B, T, C, H, W = x.shape
    x = x.contiguous()
    if out is None:
        out = torch.empty((B, T, H, W, C), dtype=torch.uint8, device=x.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (B, T, H, W, C) or out.device != x.device or not out.is_contiguous():
        raise _lib.VarsepHipError('frames_to_u8_nhwc: out must be a contiguous uint8 %s tensor on %s (got %s %s on %s, strides %s)'
                                  % ((B, T, H, W, C), x.device, out.dtype, tuple(out.shape), out.device, tuple(out.stride())))
    if out.numel():
        # the kernel stores four bytes at a time: a slice that starts off a 4-byte boundary (odd frame sizes) is filled through a fresh,
        # aligned tensor and one device copy
        dst = out if out.data_ptr() % 4 == 0 else torch.empty_like(out)
        check(_lib.load_library().vs_frames_to_u8_nhwc(x.data_ptr(), dtype_code(x), B * T, C, H * W, dst.data_ptr(), stream_ptr()),
              'vs_frames_to_u8_nhwc')
        if dst is not out:
            out.copy_(dst)
    return out


# ---- DEFLATE compression and CRC-32 on the device (csrc/vs_deflate.hip) -------------------------------------------------------------
DEFLATE_CHUNK = 32768             # VS_DEFLATE_MAX_CHUNK: bytes per independent chunk (one wave each)
DEFLATE_MIN_CHUNK = 1024          # VS_DEFLATE_MIN_CHUNK
DEFLATE_SLOT_EXTRA = 10           # VS_DEFLATE_SLOT_EXTRA: worst case of a chunk beyond its own bytes
DEFLATE_SLAB_BYTES = 256 << 20    # input bytes compressed per pass: slots + packed output stay below about 1 GiB whatever the array's size
CRC_PIECE = 1 << 16               # bytes per wave of vs_crc32
DEFLATE_MATCHERS = ('runs', 'window')
DEFLATE_MAX_HISTORY = 32768       # VS_DEFLATE_MAX_HISTORY: bytes before a slab that the window matcher may match against
DEFLATE_WINDOW_GROUP_BYTES = 4 * DEFLATE_CHUNK   # VS_DEFLATE_WINDOW_GROUP_BYTES: workspace of one workgroup of vs_deflate_chunks_window
DEFLATE_WINDOW_GROUPS = 512       # workgroups of vs_deflate_chunks_window at most (one per CU is resident: 256 CUs, two rounds): 64 MiB


def _as_bytes(t, what):
    require_cuda(t)
    if not t.is_contiguous():
        raise _lib.VarsepHipError('%s: a contiguous tensor is expected (got strides %s of shape %s)' % (what, tuple(t.stride()), tuple(t.shape)))
    return t.reshape(-1).view(torch.uint8)


def deflate_raw_slabs(t, chunk_bytes=None, slab_bytes=None, match='runs'):
    """Iterator form of deflate_raw: yields (packed uint8 [bytes] on the device, n_chunks) for one slab of at most `slab_bytes` of input
    after the other (default DEFLATE_SLAB_BYTES, rounded down to whole chunks), so that a writer can stream an array of any size to a file
    with a bounded workspace.  The pieces concatenate by bytes.  An empty tensor yields nothing.  match='window': every slab after the
    first passes the min(32768, its offset) bytes before it as history, so matches cross slab borders as they cross chunk borders."""
    if match not in DEFLATE_MATCHERS:
        raise _lib.VarsepHipError("deflate_raw: match=%r: 'runs' or 'window' expected" % (match,))
    data = _as_bytes(t, 'deflate_raw')
    chunk = DEFLATE_CHUNK if chunk_bytes is None else int(chunk_bytes)
    if chunk < DEFLATE_MIN_CHUNK or chunk > DEFLATE_CHUNK:
        raise _lib.VarsepHipError('deflate_raw: chunk_bytes %d outside %d .. %d' % (chunk, DEFLATE_MIN_CHUNK, DEFLATE_CHUNK))
    slab = max(chunk, (DEFLATE_SLAB_BYTES if slab_bytes is None else int(slab_bytes)) // chunk * chunk)
    stride = (chunk + DEFLATE_SLOT_EXTRA + 15) // 16 * 16
    n, device = data.numel(), data.device
    if n == 0:
        return
    lib = _lib.load_library()
    with torch.cuda.device(device):
        for lo in range(0, n, slab):
            part = data[lo:lo + slab]
            n_chunks = -(-part.numel() // chunk)
            slots = torch.empty((n_chunks, stride), dtype=torch.uint8, device=device)
            sizes = torch.empty((n_chunks,), dtype=torch.int64, device=device)
            e0 = _pb()
            if match == 'window':
                groups = min(n_chunks, DEFLATE_WINDOW_GROUPS)
                work = torch.empty((groups * DEFLATE_WINDOW_GROUP_BYTES // 4,), dtype=torch.int32, device=device)
                check(lib.vs_deflate_chunks_window(part.data_ptr(), min(DEFLATE_MAX_HISTORY, lo), part.numel(), chunk, slots.data_ptr(), stride,
                                                   sizes.data_ptr(), work.data_ptr(), work.numel() * 4, stream_ptr()), 'vs_deflate_chunks_window')
                _pe(e0, 'vs_deflate_chunks_window', nbytes=float(part.numel()))
            else:
                check(lib.vs_deflate_chunks(part.data_ptr(), part.numel(), chunk, slots.data_ptr(), stride, sizes.data_ptr(), stream_ptr()),
                      'vs_deflate_chunks')
                _pe(e0, 'vs_deflate_chunks', nbytes=float(part.numel()))
            ends = torch.cumsum(sizes, 0)
            offsets = ends - sizes
            total = int(ends[-1].item())
            packed = torch.empty((total,), dtype=torch.uint8, device=device)
            e0 = _pb()
            check(lib.vs_deflate_pack(slots.data_ptr(), stride, sizes.data_ptr(), offsets.data_ptr(), n_chunks, packed.data_ptr(), total,
                                      stream_ptr()), 'vs_deflate_pack')
            _pe(e0, 'vs_deflate_pack', nbytes=2.0 * total)
            yield packed, n_chunks


def deflate_raw(t, chunk_bytes=None, slab_bytes=None, match='runs'):
    """`t` (any contiguous device tensor, taken as bytes) as a raw DEFLATE stream (RFC 1951) WITHOUT its final block: (packed uint8 [bytes]
    on the device, n_chunks).  Every chunk of `chunk_bytes` (default DEFLATE_CHUNK) is compressed on its own by one wave (vs_deflate_chunks:
    literals and distance-1 run matches, stored / fixed / dynamic by exact cost) and ends on a byte boundary with an empty stored block, so
    `packed + b'\\x03\\x00'` is a complete stream that zlib inflates to t's bytes.  vs_deflate_pack gathers the chunks.  An empty tensor gives
    (empty, 0).  For arrays above DEFLATE_SLAB_BYTES prefer deflate_raw_slabs, which bounds the workspace.  match='window' adds the window
    search (vs_deflate_chunks_window: matches up to 32768 bytes back, across chunk borders; per chunk never larger than 'runs')."""
    pieces = list(deflate_raw_slabs(t, chunk_bytes, slab_bytes, match))
    if not pieces:
        return torch.empty((0,), dtype=torch.uint8, device=t.device), 0
    if len(pieces) == 1:
        return pieces[0]
    return torch.cat([p for p, _ in pieces]), sum(n for _, n in pieces)


def crc32(t, init=0):
    """zlib.crc32(bytes of t, init) as a Python int, for a contiguous device tensor of any dtype: vs_crc32 leaves one partial per piece of
    CRC_PIECE bytes (each already advanced past the bytes behind it), the host XORs the partials it reads back."""
    import numpy as np
    data = _as_bytes(t, 'crc32')
    init = int(init) & 0xFFFFFFFF
    n = data.numel()
    if n == 0:
        return init
    pieces = -(-n // CRC_PIECE)
    with torch.cuda.device(data.device):
        partial = torch.empty((pieces,), dtype=torch.int32, device=data.device)
        e0 = _pb()
        check(_lib.load_library().vs_crc32(data.data_ptr(), n, CRC_PIECE, init, partial.data_ptr(), stream_ptr()), 'vs_crc32')
        _pe(e0, 'vs_crc32', nbytes=float(n))
    return int(np.bitwise_xor.reduce(partial.cpu().numpy().view(np.uint32))) ^ 0xFFFFFFFF


# ---- chunk-parallel DEFLATE decoding on the device (csrc/vs_inflate_chunks.hip) ------------------------------------------------------
INFLATE_SLOT_BYTES = 32768        # VS_INFLATE_SLOT_BYTES: the most a segment may produce
INFLATE_REPORT_WORDS = 6          # VS_INFLATE_REPORT_WORDS: status, end, final, produced, externals, reach
INFLATE_MAX_BATCH = 2147483647    # VS_INFLATE_MAX_BATCH
INFLATE_BATCH = 4096              # candidates per launch of vs_inflate_segments: 96 KiB of workspace each, 384 MiB whatever the member's size


class InflateNotChunked:
    """What inflate_raw returns for a stream whose segments do not chain: `reason` says why, and the caller takes another route."""

    def __init__(self, reason):
        self.reason = reason

    def __repr__(self):
        return 'InflateNotChunked(%r)' % (self.reason,)


def inflate_sync_scan(comp):
    """The candidate segment starts of a raw DEFLATE stream: int64 [n] on the device, sorted -- offset 0 and every offset behind the four
    bytes 00 00 FF FF (vs_inflate_sync_scan, once to count and once to list; the sort of the short list is torch's)."""
    require_cuda(comp)
    if comp.dtype != torch.uint8 or comp.dim() != 1 or not comp.is_contiguous():
        raise _lib.VarsepHipError('inflate_sync_scan: a contiguous uint8 [bytes] tensor expected')
    lib, device, n = _lib.load_library(), comp.device, comp.numel()
    with torch.cuda.device(device):
        count = torch.zeros((2,), dtype=torch.int64, device=device)
        keep = comp if n else torch.zeros((1,), dtype=torch.uint8, device=device)
        e0 = _pb()
        check(lib.vs_inflate_sync_scan(keep.data_ptr(), n, None, 0, count.data_ptr(), stream_ptr()), 'vs_inflate_sync_scan')
        _pe(e0, 'vs_inflate_sync_scan', nbytes=float(n))
        found = int(count[0].item())
        cand = torch.empty((found,), dtype=torch.int64, device=device)
        e0 = _pb()
        check(lib.vs_inflate_sync_scan(keep.data_ptr(), n, cand.data_ptr(), found, count[1:].data_ptr(), stream_ptr()), 'vs_inflate_sync_scan')
        _pe(e0, 'vs_inflate_sync_scan', nbytes=float(n))
        return torch.sort(cand).values


def inflate_raw(comp, out_bytes, crc=None, batch=None, trace=None):
    """The `out_bytes` bytes of the raw DEFLATE stream `comp` (uint8 [bytes] on the device), decoded in parallel at its sync markers: uint8
    [out_bytes] on the device, or an InflateNotChunked when the segments do not chain (the caller then decodes the stream another way).
    Every candidate start (inflate_sync_scan) is decoded by one wave without knowing what came before it (vs_inflate_segments), `batch`
    candidates per launch (default INFLATE_BATCH) with one download of the report words per batch.  The chain is walked here: from
    candidate 0 the next segment is the candidate that starts where the last one ended; every step needs status 0, an end that is a
    candidate and no reference further back than the bytes produced so far, and the chain must close with a final segment that ends at
    the stream's last byte after exactly out_bytes.  Candidates off the chain (00 00 FF FF inside data) are decoded and ignored.  The
    chain's segments are copied to their prefix-sum offsets (vs_inflate_place) and their external bytes filled in chain order
    (vs_inflate_resolve).  crc: the CRC-32 the result must have (ops.crc32); a mismatch after a valid chain raises zipfile.BadZipFile.
    trace: optional list that receives (first candidate index, report words int64 [n, 6] as a host array) per decoded batch."""
    import numpy as np
    require_cuda(comp)
    out_bytes = int(out_bytes)
    batch = INFLATE_BATCH if batch is None else int(batch)
    if comp.dtype != torch.uint8 or comp.dim() != 1 or not comp.is_contiguous() or out_bytes < 0 or batch < 1 or batch > INFLATE_MAX_BATCH:
        raise _lib.VarsepHipError('inflate_raw: comp uint8 [bytes] contiguous, out_bytes >= 0 and batch in 1 .. %d expected' % INFLATE_MAX_BATCH)
    lib, device, n = _lib.load_library(), comp.device, comp.numel()
    S, RW = INFLATE_SLOT_BYTES, INFLATE_REPORT_WORDS
    with torch.cuda.device(device):
        cand = inflate_sync_scan(comp)
        starts = cand.cpu().numpy()
        n_cand = starts.size
        rows = min(batch, n_cand)
        out = torch.empty((max(out_bytes, 1),), dtype=torch.uint8, device=device)[:out_bytes]
        slots = torch.empty((rows, S), dtype=torch.uint8, device=device)
        marks = torch.empty((rows, S), dtype=torch.int16, device=device)
        words = torch.empty((rows, RW), dtype=torch.int64, device=device)
        total, nxt, final = 0, 0, False                                     # bytes produced, the candidate the chain is at, closed
        for lo in range(0, n_cand, batch):
            if final:
                break
            if nxt >= lo + batch:                                           # a batch of off-chain candidates only: nothing of it is needed
                continue
            m = min(batch, n_cand - lo)
            e0 = _pb()
            check(lib.vs_inflate_segments(comp.data_ptr(), n, cand[lo:].data_ptr(), m, slots.data_ptr(), S, marks.data_ptr(), words.data_ptr(),
                                          stream_ptr()), 'vs_inflate_segments')
            _pe(e0, 'vs_inflate_segments', nbytes=float(n) / max(1, -(-n_cand // batch)) + float(m) * S)
            w = words[:m].cpu().numpy()
            if trace is not None:
                trace.append((lo, w.copy()))
            plan, ext = [], []                                              # (slot, size, offset) of the chain's segments in this batch
            follow = np.searchsorted(starts, w[:, 1])                       # per candidate: the candidate that starts where it ends, if any
            is_start = (starts[np.minimum(follow, n_cand - 1)] == w[:, 1]) & (follow < n_cand)
            rows_w, follow, is_start = w.tolist(), follow.tolist(), is_start.tolist()
            while not final and lo <= nxt < lo + m:
                status, end, fin, produced, externals, reach = rows_w[nxt - lo]
                if status != 0:
                    why = 'more than %d bytes before a sync marker' % S if status == 8 else INFLATE_STATUS.get(status, 'status %d' % status)
                    return InflateNotChunked('segment at %d: %s' % (starts[nxt], why))
                if reach > total:
                    return InflateNotChunked('segment at %d reaches %d bytes back, %d bytes into the stream' % (starts[nxt], reach, total))
                if total + produced > out_bytes:
                    return InflateNotChunked('more than the %d bytes of the record' % out_bytes)
                plan.append((nxt - lo, produced, total))
                if externals:
                    ext.append(plan[-1])
                total += produced
                if fin:
                    final = True
                    if end != n:
                        return InflateNotChunked('the final block ends at %d of %d bytes' % (end, n))
                    break
                k = follow[nxt - lo]
                if not is_start[nxt - lo] or k <= nxt:
                    return InflateNotChunked('segment at %d ends at %d, which is no sync marker' % (starts[nxt], end))
                nxt = k
            for entry, table in (('vs_inflate_place', plan), ('vs_inflate_resolve', ext)):
                if not table:
                    continue
                t = torch.from_numpy(np.ascontiguousarray(np.asarray(table, dtype=np.int64).T)).to(device)
                e0 = _pb()
                if entry == 'vs_inflate_place':
                    check(lib.vs_inflate_place(slots.data_ptr(), S, m, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(table), out.data_ptr(),
                                               out_bytes, stream_ptr()), entry)
                else:
                    check(lib.vs_inflate_resolve(marks.data_ptr(), m, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(table), out.data_ptr(),
                                                 out_bytes, stream_ptr()), entry)
                _pe(e0, entry, nbytes=2.0 * sum(r[1] for r in table))
        if not final:
            return InflateNotChunked('the chain leaves the candidates before a final block')
        if total != out_bytes:
            return InflateNotChunked('%d bytes where the record says %d' % (total, out_bytes))
    if crc is not None and crc32(out) != (int(crc) & 0xFFFFFFFF):
        import zipfile
        raise zipfile.BadZipFile('inflate_raw: bad CRC-32 of %d decoded bytes' % out_bytes)
    return out


# ---- block-parallel DEFLATE decoding on the device (csrc/vs_inflate_blocks.hip) ------------------------------------------------------
INFLATE_WINDOW_BYTES = 32768      # VS_INFLATE_WINDOW_BYTES: cells a probe leaves per candidate, bytes of a window
INFLATE_BLOCKS_MAX_IN = 1 << 20   # VS_INFLATE_BLOCKS_MAX_IN: bytes of input one span may read
INFLATE_CAP = 12                  # VS_INFLATE_CAP
INFLATE_DECODE_WORDS = 3          # VS_INFLATE_DECODE_WORDS: status, end, produced


def _block_scan(entry, comp):
    """One finder (`entry`: vs_inflate_block_scan or vs_inflate_block_scan_stored) on comp: once to count and once to list, then sorted."""
    lib, device, n = _lib.load_library(), comp.device, comp.numel()
    scan = getattr(lib, entry)
    count = torch.zeros((2,), dtype=torch.int64, device=device)
    keep = comp if n else torch.zeros((1,), dtype=torch.uint8, device=device)
    e0 = _pb()
    check(scan(keep.data_ptr(), n, None, 0, count.data_ptr(), stream_ptr()), entry)
    _pe(e0, entry, nbytes=float(n))
    found = int(count[0].item())
    cand = torch.empty((found,), dtype=torch.int64, device=device)
    e0 = _pb()
    check(scan(keep.data_ptr(), n, cand.data_ptr(), found, count[1:].data_ptr(), stream_ptr()), entry)
    _pe(e0, entry, nbytes=float(n))
    return torch.sort(cand).values


def inflate_block_scan(comp, stored=False):
    """The candidate span starts of a raw DEFLATE stream without sync markers: int64 [n] BIT positions on the device, sorted -- bit 0 and
    every bit from which a non-final dynamic block header reads (vs_inflate_block_scan, once to count and once to list; the sort of the
    short list is torch's).  stored=True: the sorted union of that list and the stored finder's (vs_inflate_block_scan_stored: for every
    byte boundary B where LEN and NLEN = ~LEN stand with LEN + 1 more bytes behind them, the up to eight bit positions 8 * B - 3 - k from
    which only zero bits lead to the boundary)."""
    require_cuda(comp)
    if comp.dtype != torch.uint8 or comp.dim() != 1 or not comp.is_contiguous():
        raise _lib.VarsepHipError('inflate_block_scan: a contiguous uint8 [bytes] tensor expected')
    with torch.cuda.device(comp.device):
        cand = _block_scan('vs_inflate_block_scan', comp)
        if not stored:
            return cand
        return torch.unique(torch.cat((cand, _block_scan('vs_inflate_block_scan_stored', comp))))     # sorted, and bit 0 once


def inflate_blocks(comp, out_bytes, crc=None, batch=None, trace=None, stored=False):
    """The `out_bytes` bytes of the raw DEFLATE stream `comp` (uint8 [bytes] on the device) that has NO sync markers -- one unbroken stream
    of zlib, what np.savez_compressed stores -- decoded in parallel at its block headers: uint8 [out_bytes] on the device, or an
    InflateNotChunked when the spans do not chain (the caller then decodes the stream another way).
    Every candidate (inflate_block_scan) is probed by one wave that does not know what came before it (vs_inflate_block_probe), `batch`
    candidates per launch (default INFLATE_BATCH: 96 KiB of workspace each) with one download of the report words per batch.  The chain is
    walked here: from candidate 0 the next span is the candidate at the bit where the last one ended; every step needs status 0, an end
    that is a candidate (or a final block that ends in the stream's last byte) and no reference further back than the bytes produced so
    far, and the chain must total out_bytes.  A block end that is a candidate is a true block start, so false candidates are decoded and
    ignored.  Per batch the chain's spans get their true windows in chain order (vs_inflate_block_windows, one workgroup) and are decoded a
    second time straight into the output (vs_inflate_block_decode), whose status, end and size must be the probe's.  A span that reads more
    than INFLATE_BLOCKS_MAX_IN bytes of input before a candidate does not chain: with the dynamic finder alone long runs of stored or
    fixed blocks; with stored=True (inflate_block_scan(comp, stored=True): the stored finder's candidates too, about six of them per
    stored block, false ones probed and ignored like any other) only long runs of fixed blocks.  crc: the CRC-32 the result must have
    (ops.crc32); a mismatch after a valid chain raises zipfile.BadZipFile.  trace: optional list that receives per decoded batch a dict
    (first: first candidate index, cand: the sorted candidates as a host array, words int64 [n, 6], chain: rows of the batch on the chain,
    windows uint8 [chain + 1, 32768] and words2 int64 [chain, 3], both None where the batch has no span of the chain or the chain broke in
    it), and after a walk to the end a dict(candidates, chain, workspace_bytes), with stored=True also stored_candidates (how many
    of the candidates the dynamic finder alone does not give)."""
    import numpy as np
    require_cuda(comp)
    out_bytes = int(out_bytes)
    batch = INFLATE_BATCH if batch is None else int(batch)
    if comp.dtype != torch.uint8 or comp.dim() != 1 or not comp.is_contiguous() or out_bytes < 0 or batch < 1 or batch > INFLATE_MAX_BATCH:
        raise _lib.VarsepHipError('inflate_blocks: comp uint8 [bytes] contiguous, out_bytes >= 0 and batch in 1 .. %d expected' % INFLATE_MAX_BATCH)
    lib, device, n = _lib.load_library(), comp.device, comp.numel()
    W, RW, DW = INFLATE_WINDOW_BYTES, INFLATE_REPORT_WORDS, INFLATE_DECODE_WORDS
    with torch.cuda.device(device):
        if stored:
            dynamic = inflate_block_scan(comp)
            cand = torch.unique(torch.cat((dynamic, _block_scan('vs_inflate_block_scan_stored', comp))))
        else:
            cand = inflate_block_scan(comp)
        starts = cand.cpu().numpy()
        n_cand = starts.size
        rows = min(batch, n_cand)
        keep = comp if n else torch.zeros((1,), dtype=torch.uint8, device=device)
        out = torch.empty((max(out_bytes, 1),), dtype=torch.uint8, device=device)[:out_bytes]
        cells = torch.empty((rows, W), dtype=torch.int16, device=device)
        words = torch.empty((rows, RW), dtype=torch.int64, device=device)
        windows = torch.zeros((rows + 1, W), dtype=torch.uint8, device=device)   # row 0: the window before the batch's first span of the chain
        words2 = torch.empty((rows, DW), dtype=torch.int64, device=device)
        total, nxt, final, chain_len = 0, 0, False, 0                       # bytes produced, the candidate the chain is at, closed
        for lo in range(0, n_cand, batch):
            if final:
                break
            if nxt >= lo + batch:                                           # a batch of off-chain candidates only: nothing of it is needed
                continue
            m = min(batch, n_cand - lo)
            e0 = _pb()
            check(lib.vs_inflate_block_probe(keep.data_ptr(), n, cand.data_ptr(), n_cand, lo, m, cells.data_ptr(), words.data_ptr(), stream_ptr()),
                  'vs_inflate_block_probe')
            _pe(e0, 'vs_inflate_block_probe', nbytes=float(n) / max(1, -(-n_cand // batch)) + 2.0 * m * W)
            w = words[:m].cpu().numpy()
            rec = dict(first=lo, cand=starts, words=w.copy(), chain=[], windows=None, words2=None)
            if trace is not None:
                trace.append(rec)
            follow = np.searchsorted(starts, w[:, 1])                       # per candidate: the candidate that starts where it ends, if any
            is_start = (starts[np.minimum(follow, n_cand - 1)] == w[:, 1]) & (follow < n_cand)
            rows_w, follow, is_start = w.tolist(), follow.tolist(), is_start.tolist()
            plan = []                                                       # (row, start bit, end bit, offset, size) of the chain's spans in this batch
            while not final and lo <= nxt < lo + m:
                status, end, fin, produced, externals, reach = rows_w[nxt - lo]
                if status != 0:
                    why = 'more than %d bytes of input before a block header that can be found' % INFLATE_BLOCKS_MAX_IN if status == INFLATE_CAP \
                        else INFLATE_STATUS.get(status, 'status %d' % status)
                    return InflateNotChunked('span at bit %d: %s' % (starts[nxt], why))
                if reach > total:
                    return InflateNotChunked('span at bit %d reaches %d bytes back, %d bytes into the stream' % (starts[nxt], reach, total))
                if total + produced > out_bytes:
                    return InflateNotChunked('more than the %d bytes of the record' % out_bytes)
                plan.append((nxt - lo, int(starts[nxt]), end, total, produced))
                total += produced
                if fin:
                    final = True
                    if (end + 7) // 8 != n:
                        return InflateNotChunked('the final block ends at bit %d of %d bytes' % (end, n))
                    break
                k = follow[nxt - lo]
                if not is_start[nxt - lo] or k <= nxt:
                    return InflateNotChunked('span at bit %d ends at bit %d, which is no candidate' % (starts[nxt], end))
                nxt = k
            if not plan:
                continue
            c = len(plan)
            chain_len += c
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(plan, dtype=np.int64).T)).to(device)
            e0 = _pb()
            check(lib.vs_inflate_block_windows(cells.data_ptr(), m, t[0].data_ptr(), t[4].data_ptr(), c, windows.data_ptr(), stream_ptr()),
                  'vs_inflate_block_windows')
            _pe(e0, 'vs_inflate_block_windows', nbytes=3.0 * c * W)
            e0 = _pb()
            check(lib.vs_inflate_block_decode(keep.data_ptr(), n, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), c, windows.data_ptr(),
                                              out.data_ptr() if out_bytes else keep.data_ptr(), out_bytes, words2.data_ptr(), stream_ptr()),
                  'vs_inflate_block_decode')
            _pe(e0, 'vs_inflate_block_decode', nbytes=float(c) * W + float(sum(r[4] for r in plan)))
            w2 = words2[:c].cpu().numpy()
            if trace is not None:
                rec.update(chain=[r[0] for r in plan], windows=windows[:c + 1].cpu().numpy(), words2=w2.copy())
            want = np.asarray([(0, r[2], r[4]) for r in plan], dtype=np.int64)
            if not np.array_equal(w2, want):
                bad = int(np.nonzero((w2 != want).any(axis=1))[0][0])
                raise _lib.VarsepHipError('inflate_blocks: the second decode of the span at bit %d reports status, end, size %s where the probe '
                                          'reported %s' % (plan[bad][1], w2[bad].tolist(), want[bad].tolist()))
            windows[0].copy_(windows[c])                                    # the window behind this batch's last span, before the next batch's first
        if trace is not None:
            trace.append(dict(candidates=int(n_cand), chain=chain_len,
                              workspace_bytes=sum(x.numel() * x.element_size() for x in (cand, cells, words, windows, words2))))
            if stored:
                trace[-1]['stored_candidates'] = int(n_cand - dynamic.numel())
        if not final:
            return InflateNotChunked('the chain leaves the candidates before a final block')
        if total != out_bytes:
            return InflateNotChunked('%d bytes where the record says %d' % (total, out_bytes))
    if crc is not None and crc32(out) != (int(crc) & 0xFFFFFFFF):
        import zipfile
        raise zipfile.BadZipFile('inflate_blocks: bad CRC-32 of %d decoded bytes' % out_bytes)
    return out


def u8_tn_to_f32_nt(x):
    """uint8 [T, N, ...] on the device -> fp32 [N, T, ...] (vs_u8_tn_to_f32_nt, csrc/vs_data.hip): what `[x[:, i].astype(np.single) for i ...]` stacks on the host."""
    require_cuda(x)
    if x.dtype != torch.uint8 or x.dim() < 2 or not x.is_contiguous():
        raise _lib.VarsepHipError('u8_tn_to_f32_nt: a contiguous uint8 tensor of at least two dimensions expected')
    T, N = int(x.shape[0]), int(x.shape[1])
    inner = x.numel() // (T * N) if T * N else 0
    with torch.cuda.device(x.device):
        out = torch.empty((N, T) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        if out.numel():
            e0 = _pb()
            check(_lib.load_library().vs_u8_tn_to_f32_nt(x.data_ptr(), T, N, inner, out.data_ptr(), stream_ptr()), 'vs_u8_tn_to_f32_nt')
            _pe(e0, 'vs_u8_tn_to_f32_nt', nbytes=5.0 * x.numel())
    return out


# ---- PNG encoding on the device (csrc/vs_png_encode.hip) ---------------------------------------------------------------------------
PNG_FILTERS = {'none': 0, 'sub': 1, 'up': 2, 'average': 3, 'paeth': 4, 'adaptive': 5}
PNG_FIXED_BYTES = 65              # 57 + 8: everything of a file but its compressed chunks


def _png_filter_mode(mode, what):
    if isinstance(mode, str) and mode in PNG_FILTERS:
        return PNG_FILTERS[mode]
    if isinstance(mode, int) and not isinstance(mode, bool) and 0 <= mode <= 5:
        return mode
    raise _lib.VarsepHipError('%s: filter %r: one of %s or a type 0..4 (5: adaptive) expected' % (what, mode, ', '.join(PNG_FILTERS)))


def _deflate_match_chunk(match, chunk_bytes, what):
    if match not in DEFLATE_MATCHERS:
        raise _lib.VarsepHipError("%s: match=%r: 'runs' or 'window' expected" % (what, match))
    chunk = DEFLATE_CHUNK if chunk_bytes is None else int(chunk_bytes)
    if chunk < DEFLATE_MIN_CHUNK or chunk > DEFLATE_CHUNK:
        raise _lib.VarsepHipError('%s: chunk_bytes %d outside %d .. %d' % (what, chunk, DEFLATE_MIN_CHUNK, DEFLATE_CHUNK))
    return DEFLATE_MATCHERS.index(match), chunk


def png_filter(pixels, mode='adaptive', out=None):
    """pixels: uint8 [n, H, W, C] on the device (contiguous, any alignment), C in 1..4 -> raw uint8 [n, H * (1 + W * C)]: the filtered rows of
    every image, each row behind its filter-type byte, in one launch of vs_png_filter.  mode: 'none' | 'sub' | 'up' | 'average' | 'paeth'
    (or 0..4) gives every row that type; 'adaptive' (5) takes per row the type with the least sum of absolute signed residuals, a tie to
    the lowest type.  out: optional uint8 [n, stride >= H * (1 + W * C)] view with contiguous rows to write into; bytes of a row of `out`
    beyond the image's are not written."""
    require_cuda(pixels, out)
    if pixels.dtype != torch.uint8 or pixels.dim() != 4 or not pixels.is_contiguous() or pixels.numel() == 0 or not 1 <= pixels.shape[3] <= 4:
        raise _lib.VarsepHipError('png_filter: a non-empty contiguous uint8 [n, H, W, C] tensor with C in 1..4 is expected (got %s %s)'
                                  % (pixels.dtype, tuple(pixels.shape)))
    code = _png_filter_mode(mode, 'png_filter')
    n, H, W, C = pixels.shape
    S = H * (1 + W * C)
    if out is not None and (out.dtype != torch.uint8 or out.dim() != 2 or out.shape != (n, S) or out.stride(1) != 1
                            or (n > 1 and out.stride(0) < S) or out.device != pixels.device):
        raise _lib.VarsepHipError('png_filter: out must be uint8 [%d, %d] with contiguous rows on %s' % (n, S, pixels.device))
    with torch.cuda.device(pixels.device):
        if out is None:
            out = torch.empty((n, S), dtype=torch.uint8, device=pixels.device)
        e0 = _pb()
        check(_lib.load_library().vs_png_filter(pixels.data_ptr(), n, H, W, C, code, out.data_ptr(), max(out.stride(0), S) if n > 1 else S,
                                                stream_ptr()), 'vs_png_filter')
        _pe(e0, 'vs_png_filter', nbytes=float(n) * (S + (2 if code == 5 else 1) * H * W * C))
    return out


def deflate_streams(raw, stream_bytes, chunk_bytes=None, match='window', groups=None):
    """raw: uint8 [n, stride >= stream_bytes] on the device with contiguous rows; the first `stream_bytes` of every row are one stream, and
    every stream is compressed on its own in ONE launch of vs_deflate_streams.  Returns (slots uint8 [n * K, slot_stride], sizes int64
    [n * K]) with K = ceil(stream_bytes / chunk_bytes): slots[s * K + k, :sizes[s * K + k]] for k < K, concatenated and closed with
    b'\\x03\\x00', is a raw DEFLATE stream that inflates to stream s.  match: 'runs' or 'window' (matches up to 32768 bytes back, inside the
    stream only).  groups: workgroups (and workspace slices) of the window parse; no output byte depends on it."""
    require_cuda(raw)
    stream_bytes = int(stream_bytes)
    if raw.dtype != torch.uint8 or raw.dim() != 2 or raw.shape[0] < 1 or stream_bytes < 1 or raw.shape[1] < stream_bytes \
            or (raw.shape[1] > 1 and raw.stride(1) != 1) or (raw.shape[0] > 1 and raw.stride(0) < stream_bytes):
        raise _lib.VarsepHipError('deflate_streams: raw uint8 [n >= 1, stride >= stream_bytes >= 1] with contiguous rows expected (got %s %s, '
                                  'stream_bytes %d)' % (raw.dtype, tuple(raw.shape), stream_bytes))
    code, chunk = _deflate_match_chunk(match, chunk_bytes, 'deflate_streams')
    n, device = raw.shape[0], raw.device
    K = -(-stream_bytes // chunk)
    stride = (chunk + DEFLATE_SLOT_EXTRA + 15) // 16 * 16
    with torch.cuda.device(device):
        slots = torch.empty((n * K, stride), dtype=torch.uint8, device=device)
        sizes = torch.empty((n * K,), dtype=torch.int64, device=device)
        work, work_bytes = None, 0
        if code == 1:
            groups = min(n * K, DEFLATE_WINDOW_GROUPS) if groups is None else max(1, int(groups))
            work = torch.empty((groups * DEFLATE_WINDOW_GROUP_BYTES // 4,), dtype=torch.int32, device=device)
            work_bytes = work.numel() * 4
        e0 = _pb()
        check(_lib.load_library().vs_deflate_streams(raw.data_ptr(), n, stream_bytes, raw.stride(0) if n > 1 else stream_bytes, chunk, code,
                                                     slots.data_ptr(), stride, sizes.data_ptr(), None if work is None else work.data_ptr(),
                                                     work_bytes, stream_ptr()), 'vs_deflate_streams')
        _pe(e0, 'vs_deflate_streams', nbytes=float(n) * stream_bytes)
    return slots, sizes


def png_assemble(raw, slots, sizes, H, W, C):
    """The framing launch (vs_png_assemble): raw uint8 [n, stride >= S] (png_filter's), slots / sizes of deflate_streams over it -> (files
    uint8 [n, file_stride], file_bytes int64 [n]); file i is files[i, :file_bytes[i]].  file_bytes[i] == -1 flags sizes that are none."""
    require_cuda(raw, slots, sizes)
    n, S = raw.shape[0], int(H) * (1 + int(W) * int(C))
    if raw.dtype != torch.uint8 or raw.dim() != 2 or n < 1 or raw.shape[1] < S or (raw.shape[1] > 1 and raw.stride(1) != 1) \
            or slots.dtype != torch.uint8 or slots.dim() != 2 or not slots.is_contiguous() or sizes.dtype != torch.int64 or sizes.dim() != 1 \
            or not sizes.is_contiguous() or sizes.numel() != slots.shape[0] or sizes.numel() % n or sizes.numel() == 0:
        raise _lib.VarsepHipError('png_assemble: raw uint8 [n, >= %d], contiguous slots uint8 [n * K, slot_stride] and sizes int64 [n * K] expected' % S)
    K = sizes.numel() // n
    stride = (PNG_FIXED_BYTES + S + DEFLATE_SLOT_EXTRA * K + 15) // 16 * 16
    with torch.cuda.device(raw.device):
        files = torch.empty((n, stride), dtype=torch.uint8, device=raw.device)
        file_bytes = torch.empty((n,), dtype=torch.int64, device=raw.device)
        e0 = _pb()
        check(_lib.load_library().vs_png_assemble(raw.data_ptr(), raw.stride(0) if n > 1 else S, slots.data_ptr(), slots.stride(0), sizes.data_ptr(), n,
                                                  int(H), int(W), int(C), K, files.data_ptr(), stride, file_bytes.data_ptr(), stream_ptr()),
              'vs_png_assemble')
        _pe(e0, 'vs_png_assemble', nbytes=float(n) * (S + 2.0 * stride))
    return files, file_bytes


def png_encode_u8(images, filter='adaptive', match='window', chunk_bytes=None):
    """images: uint8 [n, H, W, C] on the device, C in 1..4 (grey, grey + alpha, RGB, RGBA) -> (files uint8 [n, stride] on the device, sizes
    int64 [n]): files[i, :sizes[i]] is a complete non-interlaced 8-bit PNG file of image i.  Three launches with no synchronisation in
    between -- vs_png_filter (`filter`: see png_filter), vs_deflate_streams (`match`, `chunk_bytes`: see deflate_streams; one zlib stream
    per image, independent of its neighbours) and vs_png_assemble (signature, IHDR, one IDAT with its Adler-32 and CRC-32, IEND).  Copy
    `files` and `sizes` to the host once each and write files[i, :sizes[i]]."""
    require_cuda(images)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.numel() == 0 or not 1 <= images.shape[3] <= 4:
        raise _lib.VarsepHipError('png_encode_u8: a non-empty uint8 [n, H, W, C] tensor with C in 1..4 is expected (got %s %s)'
                                  % (images.dtype, tuple(images.shape)))
    _png_filter_mode(filter, 'png_encode_u8')
    _deflate_match_chunk(match, chunk_bytes, 'png_encode_u8')
    images = images.contiguous()
    n, H, W, C = images.shape
    raw = png_filter(images, filter)
    slots, chunk_sizes = deflate_streams(raw, raw.shape[1], chunk_bytes, match)
    return png_assemble(raw, slots, chunk_sizes, H, W, C)


# ---- NumPy's legacy random stream on the device (csrc/vs_mt19937.hip) ----------------------------------------------------------------
MT19937_STATE_WORDS = 625         # VS_MT19937_STATE_WORDS: key[624], pos
MT19937_MAX_COLS = 8              # VS_MT19937_MAX_COLS
MT19937_STATUS = {1: 'the state holds a pos above 624 (nothing was drawn, the state is untouched)',
                  2: 'gave up after 64 outputs per draw: the state is not a stream (it was not advanced)'}


def mt19937_randint(state, lows, highs, n_rows, out=None, validate=True):
    """state: int32 [625] on the device, the words key[624], pos of np.random.RandomState's MT19937 state (the bit patterns of its uint32
    values), advanced in place; lows / highs: k <= 8 host integers each -> int32 [n_rows, k] on the device: out[r, j] is the (r * k + j)-th
    scalar `randint(lows[j], highs[j])` of the stream, bit for bit NumPy's (vs_mt19937_randint: one workgroup, launches on one stream
    continue the sequence in their order).  validate=True reads back the launch's status word (a host sync) and raises VarsepHipError for a
    pos above 624 in the state; validate=False keeps the call free of host syncs (the caller has checked the state it uploaded)."""
    import ctypes
    require_cuda(state, out)
    lows, highs = [int(v) for v in lows], [int(v) for v in highs]
    k, n_rows = len(lows), int(n_rows)
    if state.dtype != torch.int32 or state.dim() != 1 or state.numel() != MT19937_STATE_WORDS or not state.is_contiguous():
        raise _lib.VarsepHipError('mt19937_randint: state must be a contiguous int32 [%d] tensor (key[624], pos), got %s %s with strides %s'
                                  % (MT19937_STATE_WORDS, state.dtype, tuple(state.shape), tuple(state.stride())))
    if len(highs) != k or any(not -2 ** 31 <= v < 2 ** 31 for v in lows + highs):
        raise _lib.VarsepHipError('mt19937_randint: lows and highs must be equally many int32 values (got %r and %r)' % (lows, highs))
    if n_rows < 0:
        raise _lib.VarsepHipError('mt19937_randint: n_rows %d is negative' % n_rows)
    if out is None:
        out = torch.empty((n_rows, k), dtype=torch.int32, device=state.device)
    elif out.dtype != torch.int32 or out.numel() != n_rows * k or not out.is_contiguous() or out.device != state.device:
        raise _lib.VarsepHipError('mt19937_randint: out must be a contiguous int32 tensor of %d x %d entries on %s' % (n_rows, k, state.device))
    c_lows, c_highs = (ctypes.c_int32 * max(k, 1))(*lows), (ctypes.c_int32 * max(k, 1))(*highs)
    if n_rows == 0:                                  # nothing to draw (an empty tensor has no address to hand over): only the columns are checked
        check(_lib.load_library().vs_mt19937_randint(state.data_ptr(), c_lows, c_highs, k, 0, state.data_ptr(), None, None), 'vs_mt19937_randint')
        return out
    with torch.cuda.device(state.device):
        bad = torch.zeros((1,), dtype=torch.int32, device=state.device) if validate else None
        e0 = _pb()
        check(_lib.load_library().vs_mt19937_randint(state.data_ptr(), c_lows, c_highs, k, n_rows, _ptr(out), _ptr(bad), stream_ptr()),
              'vs_mt19937_randint')
        _pe(e0, 'vs_mt19937_randint', nbytes=float(out.numel() * 4 + 2 * 4 * MT19937_STATE_WORDS))
    if validate:
        status = int(bad.item())
        if status:
            raise _lib.VarsepHipError('mt19937_randint: %s' % MT19937_STATUS.get(status, 'status %d' % status))
    return out


# ---- the stochastic Moving-MNIST trajectories on the device (csrc/vs_mmnist_walk.hip) ---------------------------------------------------
MMNIST_WALK_MAX_PRE = 5           # VS_MMNIST_WALK_MAX_PRE
MMNIST_WALK_STATUS = {1: MT19937_STATUS[1],
                      2: 'a draw rejected 4096 outputs in a row: the state is not a stream (it was not advanced)',
                      3: 'a collision took more than 64 passes (the state was not advanced)'}


def mmnist_stochastic_trajectories(state, n_traj, seq_len, lows, highs, x_max, y_max, max_speed, *, start=None, latents=False, desc_nd=None,
                                   validate=True):
    """`n_traj` trajectories of the reference's stochastic Moving-MNIST sampler (speeds redrawn at every bounce) from the NumPy stream in
    `state` (int32 [625] on the device, as for mt19937_randint; advanced in place), bit for bit the reference's: per trajectory the
    len(lows) <= 5 prefix draws randint(lows[j], highs[j]) (training: digit index, start row, start column, row speed, column speed; four:
    without the digit index), then `seq_len` steps inside 0 .. x_max rows, 0 .. y_max columns (frame - digit height / width, both >= 1)
    with speeds in [-max_speed, max_speed].  With fewer than four prefix draws `start` int32 [n_traj, 4] on the device gives the start
    states.  -> (pre int32 [n_traj, n_pre], positions int32 [seq_len, n_traj, 2], latents int32 [seq_len, n_traj, 4] or None, desc int32
    [n_traj / desc_nd, 1 + desc_nd] or None): `positions.view(seq_len, -1, desc_nd, 2)` and `desc` are what moving_mnist_place reads.
    One launch of one workgroup (vs_mmnist_stochastic_trajectories); launches on one stream continue the sequence in their order.
    validate=True reads back the launch's status word (a host sync) and raises VarsepHipError; validate=False keeps the call free of host
    syncs."""
    import ctypes
    require_cuda(state, start)
    lows, highs = [int(v) for v in lows], [int(v) for v in highs]
    n_pre, n_traj, seq_len, x_max, y_max, max_speed = len(lows), int(n_traj), int(seq_len), int(x_max), int(y_max), int(max_speed)
    if state.dtype != torch.int32 or state.dim() != 1 or state.numel() != MT19937_STATE_WORDS or not state.is_contiguous():
        raise _lib.VarsepHipError('mmnist_stochastic_trajectories: state must be a contiguous int32 [%d] tensor (key[624], pos), got %s %s with '
                                  'strides %s' % (MT19937_STATE_WORDS, state.dtype, tuple(state.shape), tuple(state.stride())))
    if len(highs) != n_pre or n_pre > MMNIST_WALK_MAX_PRE or any(not -2 ** 31 <= v < 2 ** 31 for v in lows + highs):
        raise _lib.VarsepHipError('mmnist_stochastic_trajectories: lows and highs must be equally many, at most %d, int32 values (got %r and %r)'
                                  % (MMNIST_WALK_MAX_PRE, lows, highs))
    if n_traj < 0 or seq_len < 1:
        raise _lib.VarsepHipError('mmnist_stochastic_trajectories: n_traj %d must not be negative and seq_len %d must be positive' % (n_traj, seq_len))
    if x_max < 1 or y_max < 1 or max_speed < 0:
        raise _lib.VarsepHipError('mmnist_stochastic_trajectories: x_max %d and y_max %d must be >= 1 (a digit that fills the frame along an '
                                  'axis is unsupported) and max_speed %d >= 0' % (x_max, y_max, max_speed))
    if n_pre < 4 and (start is None or start.dtype != torch.int32 or tuple(start.shape) != (n_traj, 4) or not start.is_contiguous()
                      or start.device != state.device):
        raise _lib.VarsepHipError('mmnist_stochastic_trajectories: with %d prefix draws, start must be a contiguous int32 [%d, 4] tensor on %s'
                                  % (n_pre, n_traj, state.device))
    if desc_nd is not None and (n_pre != 5 or not 1 <= int(desc_nd) <= 8 or n_traj % int(desc_nd)):
        raise _lib.VarsepHipError('mmnist_stochastic_trajectories: desc needs five prefix draws and 1 .. 8 digits per video that divide n_traj '
                                  '(got %d draws, desc_nd %r, n_traj %d)' % (n_pre, desc_nd, n_traj))
    nd = int(desc_nd) if desc_nd is not None else 0
    dev = state.device
    pre = torch.empty((n_traj, n_pre), dtype=torch.int32, device=dev)
    positions = torch.empty((seq_len, n_traj, 2), dtype=torch.int32, device=dev)
    lat = torch.empty((seq_len, n_traj, 4), dtype=torch.int32, device=dev) if latents else None
    desc = torch.empty((n_traj // nd, 1 + nd), dtype=torch.int32, device=dev) if nd else None
    c_lows, c_highs = (ctypes.c_int32 * 5)(*lows), (ctypes.c_int32 * 5)(*highs)
    fn = _lib.load_library().vs_mmnist_stochastic_trajectories
    if n_traj == 0:                                  # nothing to walk (an empty tensor has no address to hand over): only the arguments are checked
        p = state.data_ptr()
        check(fn(p, c_lows, c_highs, n_pre, 0, seq_len, x_max, y_max, max_speed, p, p, p, None, None, 0, None, None),
              'vs_mmnist_stochastic_trajectories')
        return pre, positions, lat, desc
    with torch.cuda.device(dev):
        bad = torch.zeros((1,), dtype=torch.int32, device=dev) if validate else None
        e0 = _pb()
        check(fn(state.data_ptr(), c_lows, c_highs, n_pre, n_traj, seq_len, x_max, y_max, max_speed, _ptr(start) if n_pre < 4 else None,
                 _ptr(pre) if n_pre else None, _ptr(positions), _ptr(lat), _ptr(desc), nd, _ptr(bad), stream_ptr()),
              'vs_mmnist_stochastic_trajectories')
        _pe(e0, 'vs_mmnist_stochastic_trajectories', nbytes=float(4 * (pre.numel() + positions.numel()) + 2 * 4 * MT19937_STATE_WORDS))
    if validate:
        status = int(bad.item())
        if status:
            raise _lib.VarsepHipError('mmnist_stochastic_trajectories: %s' % MMNIST_WALK_STATUS.get(status, 'status %d' % status))
    return pre, positions, lat, desc

"""Every tensor derived from a parameter -- the 16-bit operand copy, the kernel-specific weight pre-packs, the eval-mode conv+BatchNorm
fold -- in ONE table:

    id(owner) -> [weakref(owner), {kind_key: [stamp, buffer]}, invalidation count]

A copy is valid for one stamp: (version counter, replay epoch, invalidation count of its row).  The version counter moves when torch or
optim.Adam updates the parameter from Python; it does NOT move when a recorded step is replayed (`increment_version` ran at capture time
only) nor when a kernel writes BatchNorm running statistics through raw pointers.  `note_replay()` (train.GraphedStep.step) and
`note_bn_update()` (every training-mode BatchNorm call) advance the epochs instead, so an eager use after replays -- evaluation between
recorded training steps, a re-recording after a learning-rate change -- re-derives what the replays have outdated.  A stale copy is
re-derived INTO THE SAME STORAGE (recorded graphs keep addressing it), and a row goes when its owner does.

`functional` re-exports the public functions below; callers use them as `functional.<name>`.
"""
import weakref

import torch

from . import ops

_EPOCH = {'replay': 0, 'bn': 0}
_TABLE = {}


def note_replay():
    """A recorded step has been replayed: parameters and BatchNorm statistics changed without moving any version counter."""
    _EPOCH['replay'] += 1
    _EPOCH['bn'] += 1


def note_bn_update():
    """A kernel rewrote running_mean / running_var through raw pointers: eval-mode folds are outdated."""
    _EPOCH['bn'] += 1


def _stamp(p, row):
    return (p._version, _EPOCH['replay'], row[2])


def _row(p, create=True):
    """The row of `p`; a row left under its id() by another tensor is not p's (and is replaced when `create`)."""
    key = id(p)
    row = _TABLE.get(key)
    if (row is None or row[0]() is not p) and create:
        row = _TABLE[key] = [weakref.ref(p, lambda r: _forget(key, r)), {}, 0]
    return row if row is not None and row[0]() is p else None


def _forget(key, ref):
    """The owner behind `ref` is gone: so is its row (unless another tensor has taken the id() since)."""
    row = _TABLE.get(key)
    if row is not None and row[0] is ref:
        _remove(key)


def _remove(key):
    row = _TABLE.pop(key)
    for t in row[1].get('fold', (None, ()))[1]:         # the fold's two tensors belong to nobody else: their rows go with it
        drop(t)


def drop(t):
    """Remove the row of tensor `t`."""
    if _row(t, create=False) is not None:
        _remove(id(t))


def _entry(p, kind_key):
    row = _row(p, create=False)
    return row[1].get(kind_key) if row is not None else None


def derived(p, kind_key, make, stamp=None, ok=None):
    """The `kind_key` copy of `p`.  `make(old buffer or None)` derives it and runs only when there is no entry of p's, its stamp is not
    the current one (`stamp`: a kind with sources besides p brings its own) or `ok(buffer)` says it no longer serves the request; what it
    returns -- the old buffer, written in place, wherever recorded graphs may address it -- is the copy from then on."""
    row = _row(p)
    stamp = _stamp(p, row) if stamp is None else stamp
    ent = row[1].get(kind_key)
    if ent is None:
        ent = row[1][kind_key] = [stamp, make(None)]
    elif ent[0] != stamp or (ok is not None and not ok(ent[1])):
        ent[1] = make(ent[1])
        ent[0] = stamp
    return ent[1]


def stale(requests):
    """requests = [(p, kind_key)] -> [(p, kind_key, old buffer or None)] for those `derived` would re-derive, in request order."""
    out = []
    for p, kind_key in requests:
        row = _row(p)
        ent = row[1].get(kind_key)
        if ent is None or ent[0] != _stamp(p, row):
            out.append((p, kind_key, None if ent is None else ent[1]))
    return out


def store(p, kind_key, buf):
    """`buf` holds the `kind_key` copy of p's current value."""
    row = _row(p)
    row[1][kind_key] = [_stamp(p, row), buf]


def invalidate(params):
    """Every copy of every kind of `params` is stale from now on (and keeps its storage)."""
    for p in params:
        row = _row(p, create=False)
        if row is not None:
            row[2] += 1


def _compute_dtype():
    from .functional import compute_dtype       # (functional imports this module)
    return compute_dtype()


# ------------------------------------------------------------------------------------------------ the 16-bit operand copy
# ONE per parameter whatever its dtype: optim.Adam rewrites it in the pass that updates the parameter (shadow_buffer_for_update).
def shadow(p, dtype):
    """Parameter as a GEMM operand: itself in fp32 mode, a cached bf16 copy (refreshed on version change) otherwise."""
    if dtype == torch.float32:
        return p.detach()

    def cast(old):
        return ops.cast(p.detach(), dtype, out=old if old is not None and old.shape == p.shape and old.dtype == dtype else None)

    return derived(p, 'shadow', cast, ok=lambda buf: buf.data_ptr() != 0 and buf.dtype == dtype)


def adopt_shadow(p, buf):
    """Make `buf` (a 16-bit tensor of p's shape, e.g. a view into the sharded optimizer's arena: parallel.GradAllReducer) THE operand copy
    of `p`: filled from the current fp32 value now, rewritten in place by the optimizer launches and the arena's all-gather afterwards."""
    assert buf.shape == p.shape and buf.dtype in (torch.bfloat16, torch.float16) and buf.is_contiguous()
    ops.cast(p.detach(), buf.dtype, out=buf)
    store(p, 'shadow', buf)


def shadow_buffer_for_update(p):
    """The live bf16 operand copy of `p`, if one exists: the optimizer kernel rewrites it in the pass that updates `p`."""
    ent = _entry(p, 'shadow')
    if ent is not None and ent[1].shape == p.shape and ent[1].dtype in (torch.bfloat16, torch.float16) and ent[1].is_contiguous():
        return ent[1]
    return None


def shadows_written(params):
    """Called after an optimizer kernel refreshed the shadows of `params` in place: mark them current."""
    for p in params:
        ent = _entry(p, 'shadow')
        if ent is not None:
            store(p, 'shadow', ent[1])


def refresh_shadows(params, dtype=None):
    """Re-cast every shadow in place (same storage) -- the form used inside a captured hipGraph step."""
    dtype = dtype or _compute_dtype()
    for p in params:
        ent = _entry(p, 'shadow')
        if ent is not None:
            ops.cast(p.detach(), dtype, out=ent[1])
            store(p, 'shadow', ent[1])


def invalidate_shadows(params):
    """Mark the operand copies (and every weight pre-pack) of `params` stale: their next use re-casts / re-packs into the same storage.  A
    recorded step whose optimizer does not maintain the copies itself calls this right before the capture, so that the recording contains
    the casts."""
    invalidate(params)


# ------------------------------------------------------------------------------------------------ weight pre-packs
def packed_weight(p, dtype, transpose):
    """Rollout pre-pack of a 2-D parameter (fragment order, compute dtype), cached per parameter version."""
    return derived(p, ('rollout', bool(transpose), dtype), lambda old: ops.pack_rollout_weight(p.detach().contiguous(), dtype, transpose, out=old))


def prepack_weights(requests, dtype):
    """Bring several rollout pre-packs up to date with ONE launch: requests = [(parameter, transpose)]."""
    todo = stale([(p, ('rollout', bool(tr), dtype)) for p, tr in requests])
    if todo:
        bufs = ops.pack_rollout_weights([(p.detach().contiguous(), key[1], old) for p, key, old in todo], dtype)
        for (p, key, _), buf in zip(todo, bufs):
            store(p, key, buf)


def packed_conv_weight(p, dtype, stride, pad):
    """Transposed-form pre-pack of a conv weight (ops.conv_pack_weight), cached per parameter version."""
    return derived(p, ('conv', dtype, stride, pad), lambda old: ops.conv_pack_weight(p.detach().contiguous(), dtype, stride, pad, out=old))


def packed_tap_weight(p, dtype):
    """Tap-GEMM pre-pack of a ConvTranspose2d k4 s2 p1 weight (ops.convt_tap_pack_weight), cached per parameter version."""
    return derived(p, ('tap', dtype), lambda old: ops.convt_tap_pack_weight(p.detach().contiguous(), dtype, out=old))


def packed_k3_weight(p, dtype, flip):
    """Tap-GEMM pre-pack of a Conv2d k3 s1 p1 weight (forward, or flipped / transposed for the input gradient)."""
    return derived(p, ('k3', dtype, bool(flip)), lambda old: ops.conv_k3_tap_pack_weight(p.detach().contiguous(), dtype, flip, out=old))


def packed_k4s2_weight(p, dtype):
    """Row-band pre-pack of a k4 s2 p1 weight over the parity planes of its gather operand (ops.conv_k4s2_pack_weight): a Conv2d weight
    [Cout, Cin, 4, 4] for its forward, a ConvTranspose2d weight [Cin, Cout, 4, 4] for its input gradient; cached per parameter version."""
    return derived(p, ('k4s2', dtype), lambda old: ops.conv_k4s2_pack_weight(p.detach().contiguous(), dtype, out=old))


def packed_img_weight(p, dtype, flip):
    """MFMA-fragment pre-pack of a Conv2d k3 s1 p1 weight for `ops.conv3_img16` (forward, or flipped / transposed: input gradient)."""
    return derived(p, ('img', dtype, bool(flip)), lambda old: ops.conv3_img16_pack_weight(p.detach().contiguous(), dtype, flip, out=old))


def prepack_conv3_weights(net, dtype=None):
    """Bring the row-band / few-maps pre-packs (forward and flipped) of every 3x3 stride-1 pad-1 convolution of `net` up to date with ONE
    launch per 96 packs (instead of one launch per pack at its first use: 36-67 launches per TaxiBJ / SST step, every step, because the
    optimizer changes every weight).  Called by the training step right before the forward pass; what is not stale is skipped."""
    import torch.nn as nn
    dtype = dtype or _compute_dtype()
    if dtype == torch.float32:
        return 0
    requests = []
    for m in net.modules():
        if not (isinstance(m, nn.Conv2d) and tuple(m.kernel_size) == (3, 3) and tuple(m.stride) == (1, 1) and tuple(m.padding) == (1, 1) and m.groups == 1):
            continue
        p = m.weight
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            continue
        requests += [(p, ('img', dtype, flip)) for flip in (False, True)]     # (any K: the pack pads the contraction to whole 64-channel phases)
    todo = stale(requests)
    if todo:
        bufs = ops.conv3_img16_pack_weights([(p.detach(), key[2], old) for p, key, old in todo], dtype)
        for (p, key, _), buf in zip(todo, bufs):
            store(p, key, buf)
    return len(todo)


# ---- inference: BatchNorm folded into the convolution ---------------------------------------------------------------------------------
# In `.eval()` a BatchNorm2d normalises with its RUNNING statistics, i.e. it is a fixed per-channel affine map of the convolution's
# output: act(gamma (conv(x) + b - mean) / sqrt(var + eps) + beta) = act(conv'(x) + b') with W' = W s, b' = (b - mean) s + beta,
# s = gamma / sqrt(var + eps).  The folded block is ONE kernel (the activation sits in the convolution's epilogue or in the pass that
# follows it) instead of convolution + BatchNorm pass; SURVEY section 8f rank 1.  Only without autograd (`torch.no_grad()`: the way the
# reference's evaluation scripts run, test/mnist/test.py:99) -- with gradients enabled the unfolded block is kept so that d gamma / d beta
# exist.  In the 16-bit modes the rounding points move with it: the folded weight is rounded once (instead of the weight), the convolution
# output is not stored before the affine map.
def folded_conv_bn(conv, bn):
    """(W', b') fp32 tensors of the eval-mode conv -> BatchNorm pair, cached until any of the six tensors involved changes.  The tensors
    keep their identity across refreshes (in-place update), so the operand copies / weight pre-packs keyed on them refresh themselves."""
    srcs = (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)
    stamp = (tuple(-1 if t is None else t._version for t in srcs) + tuple(0 if t is None else t.data_ptr() for t in srcs)
             + (_EPOCH['replay'], _EPOCH['bn']))

    def fold(old):
        with torch.no_grad():
            s = bn.weight.detach().float() * torch.rsqrt(bn.running_var.detach().float() + bn.eps)
            shape = (1, -1, 1, 1) if isinstance(conv, torch.nn.ConvTranspose2d) else (-1, 1, 1, 1)
            wf = conv.weight.detach().float() * s.view(shape)
            b0 = conv.bias.detach().float() if conv.bias is not None else torch.zeros_like(s)
            bf = (b0 - bn.running_mean.detach().float()) * s + bn.bias.detach().float()
            if old is not None and old[0].shape == wf.shape:
                old[0].copy_(wf)
                old[1].copy_(bf)
                return old
            return wf.contiguous(), bf.contiguous()

    # the entry dies with the weight it belongs to (models built and evaluated repeatedly in one process: tests, sweeps), and takes the
    # rows of W' and b' with it (drop)
    return derived(conv.weight, 'fold', fold, stamp=stamp)

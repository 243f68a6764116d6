"""The derived copies of a parameter (16-bit operand copy, six kernel pre-packs, eval-mode conv+BatchNorm fold) and the four
parameter registries of `functional`, through their public functions only: no GPU.

The `ops` cast / pack functions are replaced by CPU stand-ins that record their calls and honour `out=`, so every statement here is about
WHEN a copy is derived and INTO WHICH storage: a copy is valid for one (version counter, replay epoch) pair, a stale copy is re-derived
into the same storage (recorded graphs keep addressing it) and an entry dies with its tensor.
"""
import gc

import pytest
import torch

from ops_standins import StandIns
from spatiotemporal_variable_separation_amd import functional as VF

BF, HF = torch.bfloat16, torch.float16


@pytest.fixture
def rec(monkeypatch):
    s = StandIns()
    s.install(monkeypatch)
    return s


def param(seed=0, shape=(3, 5)):
    return torch.nn.Parameter(torch.randn(shape, generator=torch.Generator().manual_seed(seed)))


def bump(p):
    with torch.no_grad():
        p.add_(1.0)


# kind -> (use of the copy, the `ops` function that derives it, the arguments it gets after the source and the dtype)
KINDS = {
    'shadow': (lambda p: VF.shadow(p, BF), 'cast', ()),
    'rollout': (lambda p: VF.packed_weight(p, BF, True), 'pack_rollout_weight', (True,)),
    'conv': (lambda p: VF.packed_conv_weight(p, BF, 2, 1), 'conv_pack_weight', (2, 1)),
    'tap': (lambda p: VF.packed_tap_weight(p, BF), 'convt_tap_pack_weight', ()),
    'k3': (lambda p: VF.packed_k3_weight(p, BF, True), 'conv_k3_tap_pack_weight', (True,)),
    'k4s2': (lambda p: VF.packed_k4s2_weight(p, BF), 'conv_k4s2_pack_weight', ()),
    'img': (lambda p: VF.packed_img_weight(p, BF, False), 'conv3_img16_pack_weight', (False,)),
}


def expected(p, kind):
    v = p.detach().to(BF)
    return v if kind == 'shadow' else v.reshape(-1) * (-1 if KINDS[kind][2] == (True,) else 1)


# ---------------------------------------------------------------------------------------------------------------------- staleness
@pytest.mark.parametrize('kind', list(KINDS))
def test_a_copy_is_derived_once_and_rederived_into_the_same_storage_when_stale(rec, kind):
    use, name, extra = KINDS[kind]
    p, q = param(1), param(2)
    buf, other = use(p), use(q)
    assert [c[0] for c in rec.calls] == [name, name]
    assert rec.calls[0][1].data_ptr() == p.data_ptr() and not rec.calls[0][1].requires_grad       # p.detach() (contiguous already)
    assert rec.calls[0][2] == (BF,) + extra and rec.calls[0][3] is None
    assert torch.equal(buf, expected(p, kind))
    assert use(p) is buf and use(q) is other and len(rec.calls) == 2                              # fresh: the same tensor, no call
    address = buf.data_ptr()
    for outdate in (lambda: bump(p), VF.note_replay, lambda: VF.invalidate_shadows([p])):
        del rec.calls[:]
        outdate()
        again = use(p)
        assert len(rec.calls) == 1 and rec.calls[0][0] == name and rec.calls[0][3] is buf         # one re-derivation, `out` = the old buffer
        assert again is buf and again.data_ptr() == address
        assert torch.equal(again, expected(p, kind))
        assert use(p) is buf and len(rec.calls) == 1
    # invalidating p left q's copy alone (the replay epoch above outdated it once: bring it up to date first)
    assert use(q) is other
    del rec.calls[:]
    VF.invalidate_shadows([p])
    assert use(q) is other and rec.calls == []
    assert use(p) is buf and len(rec.calls) == 1


@pytest.mark.parametrize('kind', list(KINDS))
def test_an_entry_goes_with_its_parameter(rec, kind):
    use = KINDS[kind][0]
    p = param(3)
    use(p)
    assert rec.live() == 1
    del p, rec.calls[:]
    gc.collect()
    assert rec.live() == 0


def test_invalidate_reaches_every_kind_of_one_parameter(rec):
    p, q = param(4), param(5)
    bufs = {k: use(p) for k, (use, _, _) in KINDS.items()}
    others = {k: use(q) for k, (use, _, _) in KINDS.items()}
    del rec.calls[:]
    VF.invalidate_shadows([p])
    for k, (use, name, _) in KINDS.items():
        assert use(q) is others[k]
    assert rec.calls == []
    for k, (use, name, _) in KINDS.items():
        assert use(p) is bufs[k]
    assert sorted(c[0] for c in rec.calls) == sorted(name for _, name, _ in KINDS.values())
    assert all(c[3] is bufs[k] for c in rec.calls for k in KINDS if KINDS[k][1] == c[0])


# ---------------------------------------------------------------------------------------------------------- key discrimination
@pytest.mark.parametrize('a,b', [
    (lambda p: VF.packed_weight(p, BF, False), lambda p: VF.packed_weight(p, BF, True)),
    (lambda p: VF.packed_conv_weight(p, BF, 2, 1), lambda p: VF.packed_conv_weight(p, BF, 1, 0)),
    (lambda p: VF.packed_k3_weight(p, BF, False), lambda p: VF.packed_k3_weight(p, BF, True)),
    (lambda p: VF.packed_img_weight(p, BF, False), lambda p: VF.packed_img_weight(p, BF, True)),
    (lambda p: VF.packed_img_weight(p, BF, False), lambda p: VF.packed_img_weight(p, HF, False)),
    (lambda p: VF.packed_tap_weight(p, BF), lambda p: VF.packed_k4s2_weight(p, BF)),
    (lambda p: VF.packed_k3_weight(p, BF, True), lambda p: VF.packed_img_weight(p, BF, True)),
], ids=['transpose', 'stride_pad', 'k3_flip', 'img_flip', 'dtype', 'tap_vs_k4s2', 'k3_vs_img'])
def test_different_requests_of_one_parameter_are_separate_entries(rec, a, b):
    p = param(6)
    x, y = a(p), b(p)
    assert x is not y and x.data_ptr() != y.data_ptr() and len(rec.calls) == 2
    assert a(p) is x and b(p) is y and len(rec.calls) == 2
    bump(p)
    assert a(p) is x and b(p) is y and len(rec.calls) == 4
    assert rec.calls[2][3] is x and rec.calls[3][3] is y


# ------------------------------------------------------------------------------------------------------------ shadow specifics
def test_fp32_operand_is_the_parameter_itself(rec):
    p = param(7)
    s = VF.shadow(p, torch.float32)
    assert s.data_ptr() == p.data_ptr() and s.dtype == torch.float32 and not s.requires_grad
    assert rec.calls == [] and VF.shadow_buffer_for_update(p) is None


def test_there_is_one_operand_copy_per_parameter_whatever_its_dtype(rec):
    p = param(8)
    b = VF.shadow(p, BF)
    assert VF.shadow_buffer_for_update(p) is b
    h = VF.shadow(p, HF)
    assert h.dtype == HF and len(rec.calls) == 2 and rec.calls[1][3] is None                      # another dtype: not into the bf16 buffer
    assert VF.shadow_buffer_for_update(p) is h                                                    # ... and it REPLACED the copy
    assert VF.shadow(p, HF) is h and len(rec.calls) == 2
    b2 = VF.shadow(p, BF)
    assert b2.dtype == BF and len(rec.calls) == 3 and rec.calls[2][3] is None
    assert VF.shadow_buffer_for_update(p) is b2


def test_a_reshaped_parameter_gets_a_new_operand_copy(rec):
    p = param(9)
    b = VF.shadow(p, BF)
    p.data = torch.randn(2, 7)
    bump(p)
    b2 = VF.shadow(p, BF)
    assert b2.shape == (2, 7) and rec.calls[-1][3] is None and VF.shadow_buffer_for_update(p) is b2 and b2 is not b


# ---------------------------------------------------------------------------------------------------------- optimizer hand-off
def test_adopted_buffer_is_the_copy_and_the_optimizer_keeps_it_current(rec):
    p, q = param(10), param(11)
    arena = torch.zeros(64, dtype=BF)
    view = arena[16:31].view(3, 5)
    VF.adopt_shadow(p, view)
    assert len(rec.calls) == 1 and rec.calls[0][0] == 'cast' and rec.calls[0][3] is view and rec.calls[0][2] == (BF,)
    assert torch.equal(arena[16:31], p.detach().to(BF).reshape(-1))
    assert VF.shadow_buffer_for_update(p) is view
    assert VF.shadow(p, BF) is view and len(rec.calls) == 1
    # an optimizer kernel rewrote parameter and copy in one pass: only the stamp moves
    bump(p)
    VF.shadows_written([p, q])
    assert VF.shadow(p, BF) is view and len(rec.calls) == 1
    assert VF.shadow_buffer_for_update(q) is None                                                 # (no copy is created by the way)
    # the recorded form: re-cast in place, stale or not
    VF.refresh_shadows([p, q], BF)
    assert len(rec.calls) == 2 and rec.calls[1][3] is view
    bump(p)
    VF.refresh_shadows([p], BF)
    assert len(rec.calls) == 3 and rec.calls[2][3] is view and torch.equal(view, p.detach().to(BF))
    assert VF.shadow(p, BF) is view and len(rec.calls) == 3
    with pytest.raises(AssertionError):
        VF.adopt_shadow(p, torch.zeros(3, 5))                                                     # fp32 is no operand copy
    with pytest.raises(AssertionError):
        VF.adopt_shadow(p, torch.zeros(5, 3, dtype=BF))


def test_a_non_contiguous_copy_is_not_offered_to_the_optimizer(rec):
    p = param(12)
    with pytest.raises(AssertionError):
        VF.adopt_shadow(p, torch.zeros(5, 3, dtype=BF).t())
    assert VF.shadow_buffer_for_update(p) is None


# ------------------------------------------------------------------------------------------------------------- prepack_weights
def test_batched_rollout_prepack_packs_only_what_is_stale_in_one_call(rec):
    a, b = param(13), param(14)
    requests = [(a, False), (a, True), (b, False)]
    VF.prepack_weights(requests, BF)
    assert len(rec.calls) == 1 and rec.calls[0][0] == 'pack_rollout_weights'
    jobs = rec.calls[0][1]
    assert [(w.data_ptr(), bool(tr), old) for w, tr, old in jobs] == [(a.data_ptr(), False, None), (a.data_ptr(), True, None), (b.data_ptr(), False, None)]
    assert not any(w.requires_grad for w, _, _ in jobs)
    VF.prepack_weights(requests, BF)
    assert len(rec.calls) == 1                                                                    # nothing stale: no call
    bufs = [VF.packed_weight(p, BF, tr) for p, tr in requests]
    assert len(rec.calls) == 1                                                                    # the single-pack function hits
    assert torch.equal(bufs[1], -a.detach().to(BF).reshape(-1)) and torch.equal(bufs[2], b.detach().to(BF).reshape(-1))
    bump(b)
    VF.prepack_weights(requests, BF)
    assert len(rec.calls) == 2 and [(w.data_ptr(), bool(tr)) for w, tr, _ in rec.calls[1][1]] == [(b.data_ptr(), False)]
    assert rec.calls[1][1][0][2] is bufs[2]
    VF.invalidate_shadows([a])
    VF.note_replay()
    VF.prepack_weights(requests, BF)
    assert len(rec.calls) == 3
    assert [(w.data_ptr(), bool(tr)) for w, tr, _ in rec.calls[2][1]] == [(a.data_ptr(), False), (a.data_ptr(), True), (b.data_ptr(), False)]
    assert all(old is buf for (_, _, old), buf in zip(rec.calls[2][1], bufs))
    assert all(VF.packed_weight(p, BF, tr) is buf for (p, tr), buf in zip(requests, bufs)) and len(rec.calls) == 3


def test_conv3_prepack_leaves_fp32_mode_and_host_weights_alone(rec):
    net = torch.nn.Sequential(torch.nn.Conv2d(4, 4, 3, 1, 1), torch.nn.Conv2d(4, 4, 3, 1, 1))
    assert VF.prepack_conv3_weights(net, torch.float32) == 0
    assert VF.prepack_conv3_weights(net, BF) == 0                                                 # not on the device: skipped
    assert rec.calls == []


# ----------------------------------------------------------------------------------------------------------------- the fold
def conv_bn(seed=0):
    torch.manual_seed(seed)
    conv, bn = torch.nn.Conv2d(4, 6, 3, 1, 1), torch.nn.BatchNorm2d(6).eval()
    with torch.no_grad():
        bn.running_mean.uniform_(-1, 1)
        bn.running_var.uniform_(0.5, 2)
        bn.weight.uniform_(0.5, 2)
        bn.bias.uniform_(-1, 1)
    return conv, bn


def folded_reference(conv, bn):
    s = bn.weight.detach() * torch.rsqrt(bn.running_var + bn.eps)
    return conv.weight.detach() * s.view(-1, 1, 1, 1), (conv.bias.detach() - bn.running_mean) * s + bn.bias.detach()


@pytest.mark.parametrize('advance', ['count_bn_calls', 'note_replay'])
def test_fold_keeps_its_tensors_across_a_statistics_change_and_their_packs_follow(rec, advance):
    conv, bn = conv_bn()
    wf, bf = VF.folded_conv_bn(conv, bn)
    w0, b0 = folded_reference(conv, bn)
    assert torch.equal(wf, w0) and torch.equal(bf, b0)
    again = VF.folded_conv_bn(conv, bn)
    assert again[0] is wf and again[1] is bf
    pack, copy = VF.packed_img_weight(wf, BF, False), VF.shadow(wf, BF)
    assert len(rec.calls) == 2
    # a kernel writes the running statistics through raw pointers: no version counter moves, the BatchNorm epoch does
    bn.running_mean.numpy()[:] += 1.0
    bn.running_var.numpy()[:] *= 2.0
    if advance == 'count_bn_calls':
        VF.count_bn_calls(bn, 1)
    else:
        VF.note_replay()
    wf2, bf2 = VF.folded_conv_bn(conv, bn)
    assert wf2 is wf and bf2 is bf
    w1, b1 = folded_reference(conv, bn)
    assert torch.equal(wf, w1) and torch.equal(bf, b1) and not torch.equal(w1, w0)
    del rec.calls[:]
    assert VF.packed_img_weight(wf, BF, False) is pack and VF.shadow(wf, BF) is copy
    assert [c[0] for c in rec.calls] == ['conv3_img16_pack_weight', 'cast'] and rec.calls[0][3] is pack and rec.calls[1][3] is copy
    assert torch.equal(pack, w1.to(BF).reshape(-1))
    # an optimizer step on the convolution: the version counter
    bump(conv.weight)
    wf3, _ = VF.folded_conv_bn(conv, bn)
    assert wf3 is wf and torch.equal(wf, folded_reference(conv, bn)[0])


def test_models_built_and_dropped_in_a_loop_leave_nothing_behind(rec):
    def one(seed):
        conv, bn = conv_bn(seed)
        wf, bf = VF.folded_conv_bn(conv, bn)
        VF.shadow(wf, BF), VF.shadow(bf, BF), VF.packed_img_weight(wf, BF, False), VF.packed_img_weight(wf, BF, True)
        VF.packed_k3_weight(wf, BF, False), VF.packed_conv_weight(wf, BF, 1, 1), VF.packed_tap_weight(wf, BF), VF.packed_k4s2_weight(wf, BF)
        VF.packed_weight(wf, BF, False)
        VF.shadow(conv.weight, BF), VF.packed_img_weight(conv.weight, BF, False)
        VF.count_bn_calls(bn, 1)
        VF.folded_conv_bn(conv, bn)
        VF.packed_img_weight(wf, BF, False)
        n = len(rec.calls)
        del rec.calls[:]
        return n, rec.live()

    counts = []
    for i in range(50):
        n, alive = one(i)
        gc.collect()
        counts.append((n, alive, rec.live()))
    assert counts == [(12, 11, 0)] * 50, counts


# --------------------------------------------------------------------------------------------------------------- registries
REGISTRIES = {
    'grad_output': (VF.set_grad_outputs, VF.grad_output, lambda p: torch.zeros(p.shape), lambda p: torch.zeros(p.shape, dtype=HF)),
    'conv_grad_output': (VF.set_conv_grad_outputs, VF.conv_grad_output, lambda p: torch.zeros(p.shape), lambda p: torch.zeros(p.shape, dtype=BF)),
    'lowp_gradient': (VF.set_lowp_gradients, VF.lowp_gradient, lambda p: torch.zeros(p.shape, dtype=BF), lambda p: torch.zeros(p.shape)),
    'fused_optimizer': (VF.set_fused_optimizer, VF.fused_optimizer, lambda p: object(), None),
}


@pytest.mark.parametrize('name', list(REGISTRIES))
def test_registry_answers_for_the_registered_parameter_only(name):
    set_, get, good, bad = REGISTRIES[name]
    p, q, r = param(20), param(21), param(22)
    vp, vq = good(p), good(q)
    try:
        set_({p: vp, q: vq})
        assert get(p) is vp and get(q) is vq and get(r) is None
        set_({q: vq})                                                                             # a new mapping replaces the old one
        assert get(p) is None and get(q) is vq
        set_(None)
        assert get(p) is None and get(q) is None
        if bad is not None:
            with pytest.raises(AssertionError):
                set_({p: bad(p)})                                                                 # wrong dtype
            with pytest.raises(AssertionError):
                set_({p: good(param(23, (5, 3)))})                                                # wrong shape
            with pytest.raises(AssertionError):
                set_({p: good(param(24, (5, 3))).t()})                                            # not contiguous
    finally:
        set_(None)
    assert get(p) is None


def test_grad_output_accepts_the_bf16_wire_image():
    p = param(25)
    v = torch.zeros(p.shape, dtype=BF)
    try:
        VF.set_grad_outputs({p: v})
        assert VF.grad_output(p) is v
    finally:
        VF.set_grad_outputs(None)


@pytest.mark.parametrize('name', list(REGISTRIES))
def test_a_recycled_id_is_not_handed_another_parameters_entry(name):
    """The registries are keyed by id(parameter): a tensor created after a registered one was collected can get its id, and must not get
    its entry.  (New with the shared registry helper for grad_output and lowp_gradient.)"""
    set_, get, good, _ = REGISTRIES[name]
    data = torch.zeros(3, 5)
    p = data.view(3, 5)
    pid = id(p)
    try:
        set_({p: good(p)})
        del p
        gc.collect()
        kept, found = [], None
        for _ in range(2000):
            t = data.view(3, 5)
            if id(t) == pid:
                found = t
                break
            kept.append(t)
        if found is not None:                                                                     # (nothing to tell apart otherwise)
            assert get(found) is None
    finally:
        set_(None)

"""The optimizer kernels of vs_optim.hip / vs_adam_math.h -- multi-tensor Adam (vs_adam_multi_scaled), the step counter, the inf / NaN scan
(vs_check_finite_multi) and the GradScaler state update (vs_loss_scale_update) -- against the references of tests/optim_refs.py: Adam
against torch.optim.Adam in double on the CPU, element by element; the scan and the scale update exactly.  The kernel matrix calls the C ABI
through ctypes tables as optim.Adam._update does, so that alignment, gradient type, `skipped`, the step word, `scale_state` and the type
of the 16-bit operand copy are chosen per case; the last group goes through optim.Adam.

Bounds (u = 2^-24, upper case = the fp64 reference; every comparison is ONE step from the same fp32 state cast to double, so drift over steps
never enters; derivation in optim_refs.adam_bounds):
    |m - M'| <= 4u max(|M|, |G|)            (+ 4u |G| when the loss scale is no power of two)
    |v - V'| <= 8u V' + 2^-149
    |p - P'| <= 2u max(|P|, |P'|) + (S / den) bound_m + 16u |upd|,   den = sqrt(V') / sqrt(1 - b2^t) + eps, S = lr / (1 - b1^t), upd = S M' / den
A bf16 gradient enters the reference as the bf16 value cast to double; with a loss scale G = g / scale in double.  The operation-by-operation
fp32 emulation of the kernel's formula uses at most 0.50 / 0.28 / 0.45 of the p / m / v bound on these very inputs
(tests/test_optim_refs_cpu.py asserts <= 0.75), so a correct kernel passes and one that is off by a few ulp of an operand does not.  The 16-bit
copy equals p.to(dtype) bit for bit; untouched memory (guard elements around every view, everything on an overflow step, everything
outside a step_ranges range) is compared as bits.

Worst observed fractions of the bounds are printed when the module ends (run with -s), together with the number of elements that differ
bitwise from the fp32 emulation (informational: the device's pow need not equal libm's).  Measured on an MI355X:
    fp32 gradient: p 0.498, m 0.274, v 0.446 of the bound;  bf16 gradient: p 0.499, m 0.270, v 0.351;
    0 of 2 962 448 elements differ bitwise from the emulation."""
import copy
import ctypes
import functools
import os

import pytest
import torch

import optim_refs as OR
from oracle.detdata import det_uniform

pytestmark = pytest.mark.gpu

_F, _B, _H = torch.float32, torch.bfloat16, torch.float16
GUARD = 8                                            # sentinel elements before and after every view
WORST = {}
EMU = {'differ': 0, 'of': 0}
GNAME = {_F: 'fp32 gradient', _B: 'bf16 gradient'}


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
    yield
    for k in sorted(WORST):
        print('\nworst %-44s %.4g' % (k, WORST[k]))
    print('\nelements that differ bitwise from the fp32 emulation (p, m or v): %d of %d' % (EMU['differ'], EMU['of']))


def _note(group, value):
    WORST[group] = max(WORST.get(group, 0.0), float(value))


def _libs():
    from spatiotemporal_variable_separation_amd import _lib
    return _lib, _lib.load_library()


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _sid(s):
    return 'noscale' if s is None else 'scale%d' % s


# ---------------------------------------------------------------------------------------------------------------- one launch
@functools.lru_cache(maxsize=None)
def _case(t, gdtype, scale, hyper, sizes=OR.SIZES, salt=0):
    """(per tensor: n, skipped, t_j, inputs, P, G, M, V, fp64 step, bounds), the step word.  Computed once, never modified."""
    lr, betas = OR.HYPER[hyper]
    tensors, step_word = OR.adam_launch(t, gdtype, scale, sizes, salt)
    return [(n, sk, tj, inp) + OR.reference_of(inp, tj, lr, betas, scale) for n, sk, tj, inp in tensors], step_word


class Launch:
    """The tensors of one launch as views into one flat buffer per operand (p, g, m, v, the 16-bit copy), each view at a 32-byte (fp32) /
    16-byte (16-bit) boundary + its element offset, with GUARD sentinel elements before and after it."""

    def __init__(self, inputs, gdtype, shadow_dtype=None, offsets=None):
        self.ns = [int(i['p'].numel()) for i in inputs]
        self.kinds = ['p', 'g', 'm', 'v'] + (['s'] if shadow_dtype is not None else [])
        dtypes = dict(p=_F, g=gdtype, m=_F, v=_F, s=shadow_dtype)
        self.start, self.before, self.dev = {}, {}, {}
        for k in self.kinds:
            offs = (offsets or {}).get(k, [0] * len(self.ns))
            cur, starts = 0, []
            for n, off in zip(self.ns, offs):
                s = (cur + GUARD + 7) // 8 * 8 + off
                starts.append(s)
                cur = s + n
            flat = torch.full(((cur + GUARD + 7) // 8 * 8,), -7.25, dtype=dtypes[k])
            if k != 's':
                for s, n, i in zip(starts, self.ns, inputs):
                    flat[s:s + n] = i[k]
            self.start[k], self.before[k], self.dev[k] = starts, flat, flat.cuda()
            assert self.dev[k].data_ptr() % 32 == 0
        self.after = None

    def view(self, k, j, src=None):
        s = self.start[k][j]
        return (self.dev[k] if src is None else src[k])[s:s + self.ns[j]]

    def run(self, lib, skipped, step_dev, lr, betas, scale_state=None, gcode=None, n_tensors=None, numel=None, eps=OR.EPS):
        _lib, _ = _libs()
        n = len(self.ns)
        VP, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int32 * n
        code = _lib.code_of(self.dev['g'].dtype) if gcode is None else gcode
        sdt = _lib.code_of(self.dev['s'].dtype) if 's' in self.dev else _lib.BF16
        tab = [VP(*[self.view(k, j).data_ptr() for j in range(n)]) for k in self.kinds]
        cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
        return lib.vs_adam_multi_scaled(n if n_tensors is None else n_tensors, cast(tab[0]), cast(tab[1]), cast(I32(*[code] * n)), cast(tab[2]),
                                        cast(tab[3]), cast(tab[4]) if 's' in self.dev else None, sdt, cast(I64(*(numel or self.ns))),
                                        cast(I32(*skipped)), step_dev.data_ptr(), lr, betas[0], betas[1], eps,
                                        None if scale_state is None else scale_state.data_ptr(), torch.cuda.current_stream().cuda_stream)

    def fetch(self):
        torch.cuda.synchronize()
        self.after = {k: self.dev[k].cpu() for k in self.kinds}
        return self.after

    def check_guards(self, what):
        for k in self.kinds:
            keep = torch.ones(self.before[k].numel(), dtype=torch.bool)
            for s, n in zip(self.start[k], self.ns):
                keep[s:s + n] = False
            assert torch.equal(_bits(self.after[k])[keep], _bits(self.before[k])[keep]), '%s: a guard element of %s changed' % (what, k)
        assert torch.equal(_bits(self.after['g']), _bits(self.before['g'])), what + ': the gradient is read-only'

    def unchanged(self):
        return all(torch.equal(_bits(self.after[k]), _bits(self.before[k])) for k in self.kinds)


def _check_tensor(L, j, item, lr, betas, scale, what):
    """Tensor j of a fetched launch against its fp64 step: bounds, the zero block, the 16-bit copy."""
    n, sk, tj, inp, P, G, M, V, ref, bounds = item
    p, m, v = (L.view(k, j, L.after) for k in ('p', 'm', 'v'))
    frac = OR.bound_fractions(p, m, v, ref, bounds)
    gname = GNAME[inp['g'].dtype]
    for k, (f, i) in frac.items():
        _note('%s: %s, fraction of the bound' % (gname, k), f)
    ep, em, ev = OR.adam_step_fp32_emulated(inp['p'], inp['g'], inp['m'], inp['v'], tj, lr, betas, OR.EPS, scale)
    EMU['differ'] += int(((_bits(ep) != _bits(p)) | (_bits(em) != _bits(m)) | (_bits(ev) != _bits(v))).sum())
    EMU['of'] += n
    for k, (f, i) in frac.items():
        assert f <= 1.0, '%s tensor %d (n %d, t %d, skipped %d): %s element %d is %.3f of its bound' % (what, j, n, tj, sk, k, i, f)
    still = (inp['g'].float() == 0) & (inp['m'] == 0) & (inp['v'] == 0)        # g = m = v = 0: p keeps its bits, the moments stay +0
    assert torch.equal(_bits(p)[still], _bits(inp['p'])[still]) and not bool(_bits(m)[still].any()) and not bool(_bits(v)[still].any()), what
    if 's' in L.kinds:
        s = L.view('s', j, L.after)
        assert torch.equal(_bits(s), _bits(p.to(s.dtype))), '%s tensor %d: the %s copy is not p rounded to nearest even' % (what, j, s.dtype)


def _step_word(value):
    return torch.tensor([value], dtype=torch.int32).cuda()


# ---------------------------------------------------------------------------------------------------------------- a. Adam against fp64
@pytest.mark.parametrize('scale', OR.SCALES, ids=_sid)
@pytest.mark.parametrize('gdtype', OR.GDTYPES, ids=['g32', 'gbf16'])
@pytest.mark.parametrize('t', OR.STEPS)
@pytest.mark.parametrize('hyper', range(len(OR.HYPER)))
def test_adam_matches_fp64_per_element(hyper, t, gdtype, scale):
    """Eleven tensors around the scalar tail, the vector / scalar switch, the 1024-element pass and the 4096-element chunk in one launch;
    `skipped` alternates 0 / 2, so the launch holds two bias corrections (t and t + 2); magnitudes 1e-6 / 1 / 1e3, zero gradients, g == m.
    The step word advances by exactly one afterwards; the loss-scale state is only read."""
    _lib, lib = _libs()
    lr, betas = OR.HYPER[hyper]
    items, step_word = _case(t, gdtype, scale, hyper)
    sdt = (None, _B, _H)[(hyper + OR.STEPS.index(t) + OR.SCALES.index(scale)) % 3]
    L = Launch([it[3] for it in items], gdtype, sdt)
    step = _step_word(step_word)
    state = None if scale is None else torch.tensor([scale, 0.0, 3.0, 5.0]).cuda()
    _lib.check(L.run(lib, [it[1] for it in items], step, lr, betas, state), 'vs_adam_multi_scaled')
    if state is None:
        _lib.check(lib.vs_adam_step_increment(step.data_ptr(), torch.cuda.current_stream().cuda_stream), 'vs_adam_step_increment')
    else:
        _lib.check(lib.vs_adam_step_increment_scaled(step.data_ptr(), state.data_ptr(), torch.cuda.current_stream().cuda_stream), 'increment')
    L.fetch()
    what = 'lr %g betas %s t %d %s %s copy %s' % (lr, betas, t, gdtype, _sid(scale), sdt)
    assert step.item() == step_word + 1, what
    if state is not None:
        assert state.tolist() == [scale, 0.0, 3.0, 5.0]
    L.check_guards(what)
    assert {it[2] for it in items} == {t, t + 2}
    for j, it in enumerate(items):
        assert it[0] < 1023 or int(((it[3]['g'].float() == 0) & (it[3]['m'] == 0) & (it[3]['v'] == 0)).sum()) >= OR.BLOCK // 2
        _check_tensor(L, j, it, lr, betas, scale, what)


@pytest.mark.parametrize('gdtype', OR.GDTYPES, ids=['g32', 'gbf16'])
@pytest.mark.parametrize('which', ['p', 'g', 'm', 'v', 's'])
def test_adam_misaligned_views_take_the_scalar_path(which, gdtype):
    """Every size with ONE operand at element offset 1, 2 and 3 of its buffer (for the bf16 gradient and the 16-bit copy the 8-byte rule
    makes these misaligned too): `aligned[j] == 0`, the scalar path, same bounds; the guard elements around every view keep their bits."""
    _lib, lib = _libs()
    hyper, t, scale = 0, 7, None
    lr, betas = OR.HYPER[hyper]
    sizes = tuple(n for n in OR.SIZES for _ in range(3))
    items, step_word = _case(t, gdtype, scale, hyper, sizes, 1)
    sdt = _B if gdtype == _F else _H
    L = Launch([it[3] for it in items], gdtype, sdt, {which: [1 + j % 3 for j in range(len(sizes))]})
    elem = L.dev[which].element_size()
    assert all(L.view(which, j).data_ptr() % (16 if elem == 4 else 8) != 0 for j in range(len(sizes)))
    _lib.check(L.run(lib, [it[1] for it in items], _step_word(step_word), lr, betas), 'vs_adam_multi_scaled')
    L.fetch()
    what = 'misaligned %s, %s' % (which, gdtype)
    L.check_guards(what)
    for j, it in enumerate(items):
        _check_tensor(L, j, it, lr, betas, scale, what)


def test_adam_overflow_step_touches_nothing():
    """scale_state = [65536, 1, ..] (found_inf set): parameters, moments, 16-bit copies and -- through vs_adam_step_increment_scaled -- the
    step word keep their bits."""
    _lib, lib = _libs()
    lr, betas = OR.HYPER[0]
    for gdtype, sdt in ((_F, _H), (_B, _B)):
        items, step_word = _case(7, gdtype, 65536.0, 0)
        L = Launch([it[3] for it in items], gdtype, sdt)
        step = _step_word(step_word)
        state = torch.tensor([65536.0, 1.0, 3.0, 5.0]).cuda()
        _lib.check(L.run(lib, [it[1] for it in items], step, lr, betas, state), 'vs_adam_multi_scaled')
        _lib.check(lib.vs_adam_step_increment_scaled(step.data_ptr(), state.data_ptr(), torch.cuda.current_stream().cuda_stream), 'increment')
        L.fetch()
        assert L.unchanged() and step.item() == step_word and state.tolist() == [65536.0, 1.0, 3.0, 5.0]


@pytest.mark.parametrize('gdtype', OR.GDTYPES, ids=['g32', 'gbf16'])
def test_adam_under_a_grid_cap_equals_the_uncapped_launch(gdtype):
    """15 chunks walked by 2 workgroups (vs_adam_set_max_blocks(2); overlap_with_backward caps at 512): bitwise the uncapped result, and
    within the bounds of fp64."""
    _lib, lib = _libs()
    lr, betas = OR.HYPER[1]
    items, step_word = _case(2, gdtype, None, 1)
    assert sum((it[0] + 4095) // 4096 for it in items) >= 9
    free, capped = Launch([it[3] for it in items], gdtype, _B), Launch([it[3] for it in items], gdtype, _B)
    sk = [it[1] for it in items]
    _lib.check(free.run(lib, sk, _step_word(step_word), lr, betas), 'vs_adam_multi_scaled')
    prev = lib.vs_adam_set_max_blocks(2)
    try:
        _lib.check(capped.run(lib, sk, _step_word(step_word), lr, betas), 'vs_adam_multi_scaled')
    finally:
        assert lib.vs_adam_set_max_blocks(prev) == 2
    free.fetch()
    capped.fetch()
    for k in free.kinds:
        assert torch.equal(_bits(free.after[k]), _bits(capped.after[k])), k
    capped.check_guards('capped')
    for j, it in enumerate(items):
        _check_tensor(capped, j, it, lr, betas, None, 'capped at 2 workgroups')


def test_adam_tensor_count_limits_and_refused_arguments():
    """64 tensors in one launch is the most; 0 and 65 tensors, an empty tensor, lr <= 0, a beta of 1 and an fp16 gradient are refused
    (VS_ERR_ARG through _lib.check) before anything is launched."""
    _lib, lib = _libs()
    lr, betas = OR.HYPER[2]
    sizes = tuple((1, 3, 5, 1023, 1025, 4, 4097, 2)[j % 8] for j in range(64))
    items, step_word = _case(1, _F, None, 2, sizes, 2)
    L = Launch([it[3] for it in items], _F, _H)
    sk = [it[1] for it in items]
    _lib.check(L.run(lib, sk, _step_word(step_word), lr, betas), 'vs_adam_multi_scaled')
    L.fetch()
    L.check_guards('64 tensors')
    for j in range(64):                                          # the first, the middle, the last and every other one
        _check_tensor(L, j, items[j], lr, betas, None, '64 tensors')

    items65 = items + items[:1]
    L65 = Launch([it[3] for it in items65], _F, _H)
    one = Launch([items[4][3]], _F, _H)
    step = _step_word(step_word)
    refused = [lambda: L.run(lib, sk, step, lr, betas, n_tensors=0), lambda: L65.run(lib, sk + sk[:1], step, lr, betas),
               lambda: one.run(lib, [0], step, lr, betas, numel=[0]), lambda: one.run(lib, [0], step, 0.0, betas),
               lambda: one.run(lib, [0], step, -lr, betas), lambda: one.run(lib, [0], step, lr, (1.0, betas[1])),
               lambda: one.run(lib, [0], step, lr, (betas[0], 1.0)), lambda: one.run(lib, [0], step, lr, betas, gcode=_lib.F16)]
    for k, call in enumerate(refused):
        with pytest.raises(_lib.VarsepHipError, match=r'failed \(-1\)'):
            _lib.check(call(), 'vs_adam_multi_scaled (refused call %d)' % k)
    L65.fetch()
    one.fetch()
    assert L65.unchanged() and one.unchanged() and step.item() == step_word
    _lib.check(one.run(lib, [0], step, lr, betas), 'vs_adam_multi_scaled')          # the same table with legal arguments runs
    one.fetch()
    assert not one.unchanged()


# ---------------------------------------------------------------------------------------------------------------- b. the inf / NaN scan
# +inf, -inf, a quiet NaN, a NaN with the sign and only the lowest payload bit set (quiet bit clear)
BAD = {_F: (0x7F800000, 0xFF800000, 0x7FC00000, 0xFF800001), _B: (0x7F80, 0xFF80, 0x7FC0, 0xFF81), _H: (0x7C00, 0xFC00, 0x7E00, 0xFC01)}
# largest finite of either sign, smallest and largest subnormal, smallest normal, -0, +0
FINE = {_F: (0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x807FFFFF, 0x00800000, 0x80000000, 0),
        _B: (0x7F7F, 0xFF7F, 0x0001, 0x807F, 0x0080, 0x8000, 0), _H: (0x7BFF, 0xFBFF, 0x0001, 0x83FF, 0x0400, 0x8000, 0)}
STATE0 = (1024.0, 0.0, 2.0, 3.0)


def _signed(bits, t):
    w = 8 * t.element_size()
    return bits - (1 << w) if bits >= 1 << (w - 1) else bits


def _poke(t, pos, bits):
    _bits(t)[pos] = _signed(bits, t)


def _guarded(n, dtype, salt, offset=0):
    """A finite tensor of n elements as a view of a buffer whose elements right before and right after the view are +inf."""
    buf = torch.zeros(n + 2 * GUARD + offset, dtype=dtype)
    s = GUARD + offset
    buf[s:s + n] = (det_uniform((n,), salt) - 0.5).to(dtype)
    buf[s - 1] = float('inf')
    buf[s + n] = float('inf')
    buf = buf.cuda()
    return buf[s:s + n]


def _scan(cases, make_state=STATE0):
    """cases: [(list of tensors, (tensor, position, bits) to plant or None)] -> the scale_state after each scan, one row per case."""
    from spatiotemporal_variable_separation_amd import ops
    states = torch.tensor([list(make_state)] * len(cases)).cuda()
    for k, (grads, plant) in enumerate(cases):
        if plant is not None:
            t, pos, bits = plant
            old = _bits(t)[pos].clone()
            _poke(t, pos, bits)
        ops.check_finite_multi(grads, states[k])
        if plant is not None:
            _bits(t)[pos] = old
    torch.cuda.synchronize()
    return states.cpu()


def _flagged(rows, start=STATE0):
    want = torch.tensor(list(start))
    want[1] = 1.0
    return [k for k in range(rows.shape[0]) if torch.equal(rows[k], want)]


@pytest.mark.parametrize('dtype', [_F, _B, _H], ids=['f32', 'bf16', 'f16'])
def test_check_finite_flags_one_bad_element_wherever_it_sits(dtype):
    """One +inf / -inf / quiet NaN / signalling-pattern NaN per scan at the vector, pass, chunk and tail positions of a 4101-element tensor;
    the infinities right outside the view are not read; only found_inf changes."""
    n = 4096 + 5
    g = _guarded(n, dtype, 3)
    assert g.data_ptr() % 16 == 0
    positions = (0, 3, 4, 1023, 1024, 4095, 4096, n - 2, n - 1)
    cases = [([g], (g, pos, bits)) for bits in BAD[dtype] for pos in positions] + [([g], None)]
    rows = _scan(cases)
    assert _flagged(rows) == list(range(len(cases) - 1)), 'scans that did not flag (or that wrote another word): %s' % (
        sorted(set(range(len(cases) - 1)) - set(_flagged(rows))),)
    assert rows[-1].tolist() == list(STATE0), 'the clean tensor (infinities right outside it) was flagged'


def test_check_finite_tensor_index_launch_count_and_misaligned_pointer():
    """The bad element in the first, a middle and the last tensor of a 64-tensor launch; in tensors 0, 63, 64, 127, 128 and 129 of a
    130-tensor list (three launches); in an fp32 tensor at element offset 1 of its buffer (scalar path)."""
    dts = (_F, _B, _H)
    grads = [_guarded((5, 1025, 4097, 3, 1, 4096)[j % 6], dts[j % 3], 10 + j) for j in range(130)]
    cases = [(grads[:64], (grads[j], grads[j].numel() - 1, BAD[grads[j].dtype][j % 4])) for j in (0, 31, 63)]
    cases += [(grads, (grads[j], grads[j].numel() // 2, BAD[grads[j].dtype][j % 4])) for j in (0, 63, 64, 127, 128, 129)]
    cases += [(grads[:64], None), (grads, None)]
    rows = _scan(cases)
    assert _flagged(rows) == list(range(9)) and rows[9].tolist() == list(STATE0) and rows[10].tolist() == list(STATE0)
    n = 4096 + 5
    m = _guarded(n, _F, 7, offset=1)
    assert m.data_ptr() % 16 == 4
    cases = [([m], (m, pos, bits)) for bits in BAD[_F] for pos in (0, 3, 4, 4095, n - 1)] + [([m], None)]
    rows = _scan(cases)
    assert _flagged(rows) == list(range(len(cases) - 1)) and rows[-1].tolist() == list(STATE0)


@pytest.mark.parametrize('dtype', [_B, _H], ids=['bf16', 'f16'])
def test_check_finite_walks_past_its_4096_workgroups(dtype):
    """4097 * 4096 + 3 elements are 4098 chunks for a grid of 4096: the first chunk of the second pass and the very last element."""
    n = 4097 * 4096 + 3
    g = torch.zeros(n, dtype=dtype, device='cuda')
    rows = _scan([([g], (g, 4096 * 4096, BAD[dtype][0])), ([g], (g, n - 1, BAD[dtype][3])), ([g], None)])
    assert _flagged(rows) == [0, 1] and rows[2].tolist() == list(STATE0)


@pytest.mark.parametrize('dtype', [_F, _B, _H], ids=['f32', 'bf16', 'f16'])
def test_check_finite_leaves_finite_values_alone_and_never_clears(dtype):
    """The largest finite value of either sign, subnormals, the smallest normal and -0 are finite; a clean scan leaves found_inf as it was,
    0 or 1 (the flag is sticky: only loss_scale_update clears it)."""
    n = 4096 + 5
    for offset in (0, 1):
        g = _guarded(n, dtype, 5, offset)
        pattern = torch.tensor([_signed(b, g) for b in FINE[dtype]], dtype=_bits(g).dtype).repeat(n // len(FINE[dtype]) + 1)[:n]
        _bits(g).copy_(pattern.cuda())
        assert bool(torch.isfinite(g.float()).all()) and g.float().abs().max().item() == {_F: 3.4028234663852886e38, _B: 3.3895313892515355e38, _H: 65504.0}[dtype]
        assert _scan([([g], None)])[0].tolist() == list(STATE0)
        set_already = (1024.0, 1.0, 2.0, 3.0)
        assert _scan([([g], None)], set_already)[0].tolist() == list(set_already)
        rows = _scan([([g], (g, n - 1, BAD[dtype][0]))], set_already)
        assert rows[0].tolist() == list(set_already)


# ---------------------------------------------------------------------------------------------------------------- c. the scale update
def test_loss_scale_update_follows_grad_scaler_exactly():
    """vs_loss_scale_update call by call against optim_refs.grad_scaler_update (== torch's own kernel, tests/test_optim_refs_cpu.py): overflow
    at tracker 0 and mid-interval, growth exactly at the interval, the skipped-step count, found_inf cleared by every call, growth intervals
    1 / 2 / 3, backoff 0.5 / 0.25 -- and a scale that cannot grow any further stays finite (2^127 * 2 is not stored) while the tracker restarts."""
    from spatiotemporal_variable_separation_amd import ops
    runs = []
    for start, growth, backoff, interval, script in OR.scaler_cases():
        state = torch.tensor(start).cuda()
        want, got = list(start), []
        expect = []
        for inf in script:
            state[1] = float(inf)
            ops.loss_scale_update(state, growth, backoff, interval)
            got.append(state.clone())
            want[1] = float(inf)
            want = OR.grad_scaler_update(want, growth, backoff, interval)
            expect.append(list(want))
        runs.append((start, growth, backoff, interval, got, expect))
    torch.cuda.synchronize()
    for start, growth, backoff, interval, got, expect in runs:
        got = [g.tolist() for g in got]
        print('loss_scale_update from %s (growth %g, backoff %g, interval %d): scales %s' % (start, growth, backoff, interval, [g[0] for g in got]))
        assert got == expect, (start, growth, backoff, interval)


# ---------------------------------------------------------------------------------------------------------------- d. through optim.Adam
def _grad(shape, step, i):
    return ((det_uniform(shape, 200 + 10 * step + i) - 0.5) * 10.0 ** (step - 2)).cuda()


def _five_steps(resume):
    from spatiotemporal_variable_separation_amd.optim import Adam
    shapes = [(4097,), (33, 7), (5,)]
    ps = [torch.nn.Parameter((det_uniform(s, 70 + i) - 0.5).cuda()) for i, s in enumerate(shapes)]
    opt = Adam(ps, lr=1e-3, betas=(0.9, 0.999))
    for step in range(5):
        if resume and step == 3:
            saved = copy.deepcopy(opt.state_dict())               # what torch.save / torch.load hand to the resumed run
            ps = [torch.nn.Parameter(p.detach().clone()) for p in ps]
            opt = Adam(ps, lr=1e-3, betas=(0.9, 0.999))
            opt.load_state_dict(saved)
        for i, p in enumerate(ps):
            p.grad = None if (step == 1 and i == 1) else _grad(p.shape, step, i)
        opt.step()
    torch.cuda.synchronize()
    return ps, opt.state_dict()


def test_resumed_run_equals_the_uninterrupted_run_bitwise():
    """state_dict() after three steps -> load_state_dict() into a fresh Adam over cloned parameters -> two more steps == five steps in one
    go, bitwise, in the parameters, both moments and the per-parameter step (the second parameter sat out the second step: load_state_dict
    drops the device step word and _init_group rebuilds it and the per-tensor lag from the saved per-parameter steps)."""
    pa, sa = _five_steps(False)
    pb, sb = _five_steps(True)
    assert [float(sa['state'][k]['step']) for k in range(3)] == [5.0, 4.0, 5.0]
    for k in range(3):
        assert float(sb['state'][k]['step']) == float(sa['state'][k]['step']), k
        assert torch.equal(_bits(pa[k].detach()), _bits(pb[k].detach())), k
        for name in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(_bits(sa['state'][k][name]), _bits(sb['state'][k][name])), (k, name)


def test_130_parameters_in_one_group_match_fp64():
    """Three launches (64 + 64 + 2 tensors) from one step(): every parameter within the bounds of its fp64 step."""
    from spatiotemporal_variable_separation_amd.optim import Adam
    lr, betas = OR.HYPER[0]
    p0, g0 = zip(*[OR.first_step_tensor(j) for j in range(130)])
    sizes = [p.numel() for p in p0]
    ps = [torch.nn.Parameter(p.cuda()) for p in p0]
    for p, g in zip(ps, g0):
        p.grad = g.cuda()
    opt = Adam(ps, lr=lr, betas=betas)
    opt.step()
    torch.cuda.synchronize()
    assert opt.param_groups[0]['step_dev'].item() == 1
    for j, (p, g) in enumerate(zip(p0, g0)):
        z = torch.zeros_like(p, dtype=torch.float64)
        ref = OR.adam_step_fp64(p, g, z, z, 1, lr, betas, OR.EPS)
        bounds = OR.adam_bounds(p.double(), g.double(), z, ref)
        st = opt.state[ps[j]]
        frac = OR.bound_fractions(ps[j].detach(), st['exp_avg'], st['exp_avg_sq'], ref, bounds)
        for k, (f, i) in frac.items():
            _note('fp32 gradient: %s, fraction of the bound' % k, f)
            assert f <= 1.0, (j, sizes[j], k, i, f)


def test_step_ranges_updates_its_range_and_nothing_else():
    """step_ranges([(p, lo, hi)]) with an fp32 gradient: inside lo..hi-1 bitwise a full step_subset on a clone, outside it p, m and v keep
    their bits."""
    from spatiotemporal_variable_separation_amd.optim import Adam
    n = 3 * 4096 + 40
    runs = []
    for _ in range(2):
        p = torch.nn.Parameter((det_uniform((n,), 81) - 0.5).cuda())
        opt = Adam([p], lr=1e-3, betas=(0.9, 0.99))
        p.grad = _grad((n,), 2, 0)
        opt.step()                                               # non-zero moments, device step 1
        p.grad = _grad((n,), 2, 1)
        runs.append((p, opt))
    (pa, oa), (pb, ob) = runs
    before = [x.detach().clone() for x in (pa, oa.state[pa]['exp_avg'], oa.state[pa]['exp_avg_sq'])]
    for lo, hi in ((8, 16), (4096 - 8, 2 * 4096 + 24), (n - 8, n)):
        oa.step_ranges([(pa, lo, hi)])
    ob.step_subset([pb])
    torch.cuda.synchronize()
    inside = torch.zeros(n, dtype=torch.bool, device='cuda')
    for lo, hi in ((8, 16), (4096 - 8, 2 * 4096 + 24), (n - 8, n)):
        inside[lo:hi] = True
    pairs = ((pa.detach(), pb.detach()), (oa.state[pa]['exp_avg'], ob.state[pb]['exp_avg']), (oa.state[pa]['exp_avg_sq'], ob.state[pb]['exp_avg_sq']))
    for (a, b), old in zip(pairs, before):
        assert torch.equal(_bits(a)[inside], _bits(b)[inside])
        assert torch.equal(_bits(a)[~inside], _bits(old)[~inside])
        assert not torch.equal(_bits(b)[~inside], _bits(old)[~inside])
    assert oa.param_groups[0]['step_dev'].item() == 1           # neither advances the step word


def test_gemm_adam_with_a_lagging_step_count_equals_gemm_then_adam():
    """ops.gemm_adam with skipped = 2 at device step 5 (the weight takes its 4th step): bitwise ops.gemm followed by a C-ABI Adam launch
    with the same `skipped`, and within the bounds of the fp64 step at t = 4 -- not t = 6."""
    from spatiotemporal_variable_separation_amd import ops
    _lib, lib = _libs()
    M, N, K = 136, 264, 40
    lr, betas = 4e-4, (0.9, 0.99)
    p0 = det_uniform((M, N), 3) - 0.5
    m0 = (det_uniform((M, N), 4) - 0.5) * 0.1
    v0 = (0.05 + det_uniform((M, N), 5)).pow(2) * 0.01
    dz = ((det_uniform((K, M), 10) - 0.5) * 0.1).cuda().to(_B)
    h = (det_uniform((K, N), 20) - 0.5).cuda().to(_B)
    step = _step_word(5)
    pa, ma, va = p0.cuda(), m0.cuda(), v0.cuda()
    sa = torch.zeros((M, N), dtype=_B, device='cuda')
    ops.gemm_adam(dz, 1, h, 1, M, N, K, pa, ma, va, sa, step, 2, lr, betas, OR.EPS)
    os.environ['VS_GEMM_MID'] = '2'                              # the tile of the fused kernel, no split-K: the same sums in the same order
    os.environ['VS_GEMM_BIG'] = '0'
    try:
        grad = ops.gemm(dz, 1, h, 1, M, N, K)
    finally:
        del os.environ['VS_GEMM_MID'], os.environ['VS_GEMM_BIG']
    torch.cuda.synchronize()
    inp = dict(p=p0.flatten(), g=grad.cpu().flatten(), m=m0.flatten(), v=v0.flatten())
    L = Launch([inp], _F, _B)
    _lib.check(L.run(lib, [2], step, lr, betas), 'vs_adam_multi_scaled')
    L.fetch()
    assert step.item() == 5
    for k, fused in (('p', pa), ('m', ma), ('v', va), ('s', sa)):
        assert torch.equal(_bits(L.view(k, 0, L.after)), _bits(fused.cpu().flatten())), k
    item = (M * N, 2, 4, inp) + OR.reference_of(inp, 4, lr, betas, None)
    _check_tensor(L, 0, item, lr, betas, None, 'gemm_adam, skipped 2')
    wrong = OR.reference_of(inp, 6, lr, betas, None)
    assert OR.bound_fractions(pa.cpu().flatten(), ma.cpu().flatten(), va.cpu().flatten(), wrong[4], wrong[5])['p'][0] > 1.0

"""GPU: the two training renderers of Moving MNIST, vs_moving_mnist_batch (walks the draws) and vs_moving_mnist_place (reads tables), which
share the loaders, the plan and the compositor of the test-set renderers (csrc/vs_data.hip): every output type, chunked and whole-video
plans, frames that 16-byte stores do not tile, rectangular digits, tables that name what is not there, guard bytes round the outputs at
aligned and shifted pointers, and a draw that names a digit past the end.  References: oracle.mmnist_ref.render and the NumPy placement of
tests/test_eval_cli_gpu.py; exact for fp32, torch's conversion of the fp32 reference for the 16-bit types."""
import functools

import numpy as np
import pytest
import torch

from guard_util import guarded_ops
from oracle import mmnist_ref

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SPEED = 4
# (F, (digit h, w), nd, B, T): few videos of many frames; the digit limit; F * F a multiple of 4 and of no more (fp32 vectors cross row
# ends, 16-bit goes element by element); element form throughout; a rectangular digit; the test-set renderers' threshold of 512 videos;
# and the training renderers' own of 2 048, from which on a workgroup renders a whole video
BATCH_SHAPES = [(64, (28, 28), 2, 3, 17), (64, (28, 28), 8, 2, 9), (30, (28, 28), 1, 2, 9), (29, (28, 28), 2, 2, 9), (40, (30, 28), 3, 2, 12),
                (32, (12, 12), 2, 512, 3), (32, (12, 12), 2, 2048, 3)]


@functools.lru_cache(maxsize=None)
def _batch_case(F, digit, nd, B, T, n_digits=23):
    """(digits uint8 [n, h, w], init int32 [B, nd, 5], reference fp32 [B, T, 1, F, F]); shared, not to be written to."""
    rng = np.random.RandomState(F * 1000 + nd * 100 + B)
    h, w = digit
    digits = (rng.randint(0, 256, size=(n_digits, h, w)) * (rng.rand(n_digits, h, w) < 0.6)).astype(np.uint8)
    init = np.stack([rng.randint(0, n_digits, (B, nd)), rng.randint(0, F - h + 1, (B, nd)), rng.randint(0, F - w + 1, (B, nd)),
                     rng.randint(-SPEED, SPEED + 1, (B, nd)), rng.randint(-SPEED, SPEED + 1, (B, nd))], axis=2).astype(np.int32)
    if nd > 1:
        init[0, 1, 1:] = init[0, 0, 1:]                                        # two digits travel together: sums over 255, clipped
    ref = mmnist_ref.render(digits, init, T, F)
    assert ref.dtype == np.float32
    for a in (digits, init, ref):
        a.setflags(write=False)
    return digits, init, ref


def _place_reference(digits, pos, desc, T, F, skip=()):
    """fp32 [V, T, 1, F, F]: test_eval_cli_gpu's NumPy placement; `skip` holds the (t, sequence, digit slot) that are not drawn."""
    V, nd = desc.shape[0], desc.shape[1] - 1
    h, w = digits.shape[1:]
    ref = np.zeros((V, T, 1, F, F), dtype=np.float32)
    for v in range(V):
        for t in range(T):
            for i in range(nd):
                seq, d = desc[v, 0], desc[v, 1 + i]
                if not 0 <= seq < pos.shape[1] or not 0 <= d < len(digits) or (t, seq, i) in skip:
                    continue
                sx, sy = pos[t, seq, i]
                ref[v, t, 0, sx:sx + h, sy:sy + w] += digits[d]
    ref[ref > 255] = 255
    return ref / np.float32(255)


@functools.lru_cache(maxsize=None)
def _place_case(F, nd, T=6, n_seq=3, V=7, n_digits=31):
    """(digits, positions int32 [T + 2, n_seq, nd, 2], desc int32 [V, 1 + nd], reference): 7 videos over 3 sequences, so several share one;
    the digits of a video are a permutation's worth of distinct indices; the table is longer than the videos."""
    rng = np.random.RandomState(77 * F + nd)
    digits = rng.randint(0, 256, size=(n_digits, 28, 28)).astype(np.uint8)
    pos = rng.randint(0, F - 28 + 1, size=(T + 2, n_seq, nd, 2)).astype(np.int32)
    pos[0, 0, 0] = (F - 28, F - 28)                                            # both borders touched exactly
    pos[1, 0, 0] = (0, 0)
    desc = np.stack([np.concatenate([[v % n_seq], rng.permutation(n_digits)[:nd]]) for v in range(V)]).astype(np.int32)
    ref = _place_reference(digits, pos, desc, T, F)
    for a in (digits, pos, desc, ref):
        a.setflags(write=False)
    return digits, pos, desc, ref


def _cuda(*arrays):
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', BATCH_SHAPES, ids=lambda s: 'F%d_%dx%d_nd%d_B%d_T%d' % (s[0], s[1][0], s[1][1], s[2], s[3], s[4]))
def test_batch_equals_the_oracle(shape, dtype):
    from spatiotemporal_variable_separation_amd import ops
    F, _, _, B, T = shape
    digits, init, ref = _batch_case(*shape)
    out = ops.moving_mnist_batch(*_cuda(digits, init), T, F, dtype)
    assert out.dtype == dtype and tuple(out.shape) == (B, T, 1, F, F)
    assert torch.equal(out.cpu(), torch.tensor(ref).to(dtype))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('F,nd', [(64, 1), (64, 2), (64, 3), (29, 2)])
def test_place_equals_the_numpy_placement(F, nd, dtype):
    from spatiotemporal_variable_separation_amd import ops
    digits, pos, desc, ref = _place_case(F, nd)
    T = pos.shape[0] - 2
    out = ops.moving_mnist_place(*_cuda(digits, pos, desc), T, F, dtype)
    assert out.dtype == dtype and tuple(out.shape) == ref.shape
    assert torch.equal(out.cpu(), torch.tensor(ref).to(dtype))


@pytest.mark.parametrize('dtype', DTYPES)
def test_place_leaves_out_what_a_bad_table_names_and_says_so(dtype):
    """One table with a sequence index out of range, a digit index out of range and a digit one pixel over each border of the frame."""
    from spatiotemporal_variable_separation_amd import _lib, ops
    F, nd = 64, 2
    digits, pos, desc, _ = _place_case(F, nd)
    pos, desc = pos.copy(), desc.copy()
    T, room = pos.shape[0] - 2, F - 28
    desc[1, 0] = pos.shape[1]                                                  # video 1: no such sequence
    desc[2, 1] = len(digits)                                                   # video 2: its first digit is past the end
    over = {(0, 1, 0): (-1, 5), (1, 1, 1): (5, -1), (2, 2, 0): (room + 1, 5), (3, 2, 1): (5, room + 1)}
    for (t, seq, i), p in over.items():
        pos[t, seq, i] = p
    ref = _place_reference(digits, pos, desc, T, F, skip=set(over))
    assert (ref[1] == 0).all() and ref[2].any()
    operands = _cuda(digits, pos, desc)
    with pytest.raises(_lib.VarsepHipError, match='out of range or a digit does not lie inside'):
        ops.moving_mnist_place(*operands, T, F, dtype)
    out = ops.moving_mnist_place(*operands, T, F, dtype, validate=False)
    assert torch.equal(out.cpu(), torch.tensor(ref).to(dtype))


@pytest.mark.parametrize('F,dtype', [(64, torch.float32), (64, torch.bfloat16), (29, torch.float32)])
@pytest.mark.parametrize('entry', ['batch', 'place'])
def test_outputs_stay_inside_their_windows_at_aligned_and_shifted_pointers(entry, F, dtype, monkeypatch):
    """The output between two 4 KiB bands of 0xFF (tests/guard_util.py), 16-byte aligned and one element off, which forces the element
    form: no byte outside the window changes, every element inside is written, and both forms give the same frames."""
    from spatiotemporal_variable_separation_amd import ops
    if entry == 'batch':
        digits, init, ref = _batch_case(F, (28, 28), 2, 3 if F == 64 else 2, 17 if F == 64 else 9)
        operands = _cuda(digits, init)
        run = lambda: ops.moving_mnist_batch(*operands, ref.shape[1], F, dtype)                                    # noqa: E731
    else:
        digits, pos, desc, ref = _place_case(F, 2)
        operands = _cuda(digits, pos, desc)
        run = lambda: ops.moving_mnist_place(*operands, ref.shape[1], F, dtype, validate=False)                    # noqa: E731
    want = torch.tensor(ref).to(dtype)
    esize = want.element_size()
    for misalign in (0, 1):
        with monkeypatch.context() as patch:
            allocs = guarded_ops(patch, misalign=misalign)
            out = run()
        assert len(allocs.guards) == 1 and out.data_ptr() % 16 == misalign * esize
        allocs.check()
        allocs.guards[0].assert_written(out)
        assert torch.equal(out.cpu(), want)


def test_a_draw_that_names_a_digit_past_the_end_draws_nothing():
    """Through the C ABI (ops does not read `init` back): digit indices n_digits_total, 2^31 - 1 and -1.  The images of such digits are
    zeros in LDS and `digits` is never indexed with them: the launch completes and the other digits are where the oracle puts them."""
    from spatiotemporal_variable_separation_amd import _lib
    F, T = 64, 9
    digits, init, _ = _batch_case(F, (28, 28), 2, 3, 17)
    init = init.copy()
    n = len(digits)
    init[0, 0, 0], init[1, 1, 0], init[2, 0, 0] = n, 2 ** 31 - 1, -1
    shown = init.copy()
    shown[..., 0] = np.where((init[..., 0] >= 0) & (init[..., 0] < n), init[..., 0], n)                            # a black image at index n
    ref = mmnist_ref.render(np.concatenate([digits, np.zeros((1, 28, 28), np.uint8)]), shown, T, F)
    d_digits, d_init = _cuda(digits, init)
    out = torch.empty((3, T, 1, F, F), dtype=torch.float32, device='cuda')
    _lib.check(_lib.load_library().vs_moving_mnist_batch(d_digits.data_ptr(), n, 28, 28, d_init.data_ptr(), 3, 2, T, F, out.data_ptr(), _lib.F32,
                                                         _lib.stream_ptr()), 'vs_moving_mnist_batch')
    assert torch.equal(out.cpu(), torch.tensor(ref))

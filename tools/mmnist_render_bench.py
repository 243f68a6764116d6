"""Per-launch times of the four Moving-MNIST renderers and of the stochastic walk, of THIS tree's library against another build of the
library (the parent commit's), through the C ABI with the same arguments: both libraries are loaded into one process and measured in
alternating windows, so that drift of the box is shared.  Every case also compares the two libraries' outputs bit for bit.  Writes the
note given by --out (default profiles/mmnist_render_timing.md).

    python tools/mmnist_render_bench.py --parent-lib PATH/libvarsep_hip.so [--lib PATH] [--out FILE] [--label NAME]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from spatiotemporal_variable_separation_amd import _lib  # noqa: E402

REPS = 9
N_DIGITS, H, F, ND, SPEED = 10000, 28, 64, 2, 4
BAR = 1.10


def load(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def windows(fns, launches):
    """[(median, min, max) microseconds per launch] per fn, over REPS windows of `launches` launches each, the fns taking turns."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(REPS):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(1e3 * e0.elapsed_time(e1) / launches)
    return [(float(np.median(t)), min(t), max(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', required=True, help='libvarsep_hip.so built from the parent commit')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mmnist_render_timing.md'))
    ap.add_argument('--lib', default=_lib.LIB_PATH, help='the library measured against the parent (default: this tree\'s)')
    ap.add_argument('--label', default='this tree')
    args = ap.parse_args()
    libs = [load(args.parent_lib), load(args.lib)]
    dev = torch.device('cuda', 0)
    stream = _lib.stream_ptr()
    g = torch.Generator(device='cpu').manual_seed(5)
    digits = (torch.randint(0, 256, (N_DIGITS, H, H), generator=g, dtype=torch.uint8) * (torch.rand((N_DIGITS, H, H), generator=g) < 0.2)).to(dev)
    room = F - H

    def draws(n):
        cols = [torch.randint(0, N_DIGITS, (n, ND, 1), generator=g), torch.randint(0, room + 1, (n, ND, 2), generator=g),
                torch.randint(-SPEED, SPEED + 1, (n, ND, 2), generator=g)]
        return torch.cat(cols, dim=2).to(torch.int32).to(dev)

    def call(lib, name, *a):
        rc = getattr(lib, name)(*a)
        if rc != 0:
            raise RuntimeError('%s failed (%d): %s' % (name, rc, lib.vs_last_error().decode()))

    cases = []                                                               # (row label, launches per window, make(lib) -> (fn, outputs))

    def batch(B, T, dtype):
        init = draws(B)

        def make(lib):
            out = torch.empty((B, T, 1, F, F), dtype=dtype, device=dev)
            return (lambda: call(lib, 'vs_moving_mnist_batch', digits.data_ptr(), N_DIGITS, H, H, init.data_ptr(), B, ND, T, F, out.data_ptr(),
                                 _lib.dtype_code(out), stream)), [out]
        return make

    def place(B, T, dtype):
        pos = torch.randint(0, room + 1, (T, B, ND, 2), generator=g).to(torch.int32).to(dev)
        desc = torch.cat([torch.arange(B).view(B, 1), torch.randint(0, N_DIGITS, (B, ND), generator=g)], dim=1).to(torch.int32).to(dev)

        def make(lib):
            out = torch.empty((B, T, 1, F, F), dtype=dtype, device=dev)
            return (lambda: call(lib, 'vs_moving_mnist_place', digits.data_ptr(), N_DIGITS, H, H, pos.data_ptr(), B, ND, desc.data_ptr(), B, T, F,
                                 out.data_ptr(), _lib.dtype_code(out), None, stream)), [out]
        return make

    def testset(V, T, fp32, placed):
        init = draws(V)
        pos = torch.randint(0, room + 1, (T, V, ND, 2), generator=g).to(torch.int32).to(dev)
        idx = init[:, :, 0].contiguous()

        def make(lib):
            out = torch.empty((V, T, 1, F, F), dtype=torch.float32, device=dev) if fp32 else torch.empty((T, V, 1, F, F), dtype=torch.uint8, device=dev)
            st, sv = (F * F, T * F * F) if fp32 else (V * F * F, F * F)
            lat = torch.empty((T, V, ND, 4), dtype=torch.int32, device=dev)
            if placed:
                return (lambda: call(lib, 'vs_moving_mnist_testset_place', digits.data_ptr(), N_DIGITS, H, H, pos.data_ptr(), idx.data_ptr(), V, ND, T,
                                     F, out.data_ptr(), int(fp32), st, sv, None, stream)), [out]
            return (lambda: call(lib, 'vs_moving_mnist_testset', digits.data_ptr(), N_DIGITS, H, H, init.data_ptr(), V, ND, T, F, out.data_ptr(),
                                 int(fp32), st, sv, lat.data_ptr(), stream)), [out, lat]
        return make

    def walk(n_traj, T, n_pre):
        cols = [(0, N_DIGITS), (0, room + 1), (0, room + 1), (-SPEED, SPEED + 1), (-SPEED, SPEED + 1)][5 - n_pre:]
        lows, highs = ((ctypes.c_int32 * 5)(*([c[k] for c in cols] + [0] * (5 - n_pre))) for k in (0, 1))
        key = torch.from_numpy(np.concatenate([np.random.RandomState(9).get_state()[1], [624]]).astype(np.uint32).view(np.int32))

        def make(lib):
            state = key.clone().to(dev)
            pre = torch.empty((n_traj, n_pre), dtype=torch.int32, device=dev)
            positions = torch.empty((T, n_traj, 2), dtype=torch.int32, device=dev)
            latents = torch.empty((T, n_traj, 4), dtype=torch.int32, device=dev)
            desc = torch.empty((n_traj // ND, 1 + ND), dtype=torch.int32, device=dev) if n_pre == 5 else None
            bad = torch.zeros((1,), dtype=torch.int32, device=dev)
            return (lambda: call(lib, 'vs_mmnist_stochastic_trajectories', state.data_ptr(), ctypes.cast(lows, ctypes.c_void_p),
                                 ctypes.cast(highs, ctypes.c_void_p), n_pre, n_traj, T, room, room, SPEED, None, pre.data_ptr(),
                                 positions.data_ptr(), latents.data_ptr(), desc.data_ptr() if desc is not None else None, ND, bad.data_ptr(),
                                 stream)), [state, pre, positions, latents, bad]
        return make

    for dtype, name in ((torch.float32, 'fp32'), (torch.bfloat16, 'bf16')):
        cases.append(('`vs_moving_mnist_batch`, B = 128 x 15 frames, %s' % name, 200, batch(128, 15, dtype)))
        cases.append(('`vs_moving_mnist_place`, B = 128 x 15 frames, %s' % name, 200, place(128, 15, dtype)))
    for fp32, name in ((False, 'uint8 [T, N, 1, F, F]'), (True, 'fp32 [N, T, 1, F, F]')):
        cases.append(('`vs_moving_mnist_testset`, 5 000 x 100 frames, %s' % name, 10, testset(5000, 100, fp32, False)))
        cases.append(('`vs_moving_mnist_testset_place`, 5 000 x 100 frames, %s' % name, 10, testset(5000, 100, fp32, True)))
    cases.append(('`vs_mmnist_stochastic_trajectories`, B = 128 (256 trajectories x 15 frames, 5 draws each)', 50, walk(256, 15, 5)))
    cases.append(('`vs_mmnist_stochastic_trajectories`, 10 000 trajectories x 100 frames, 4 draws each', 2, walk(10000, 100, 4)))

    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say('# The Moving-MNIST renderers and the stochastic walk against the parent commit (one MI355X, `tools/mmnist_render_bench.py`)')
    say()
    say('%d stand-in digits of %d x %d, frames of %d x %d, %d digits per video, speed %d.  Both libraries in one process, the same arguments '
        'through the C ABI; median (min - max) microseconds per launch over %d windows per library, the libraries taking turns window by '
        'window, warm.  The bar is %s / parent <= %.2f.' % (N_DIGITS, H, H, F, F, ND, SPEED, REPS, args.label, BAR))
    say()
    say('| launch | parent | %s | ratio | within the bar | same bits |' % args.label)
    say('|---|---|---|---|---|---|')
    worst = 0.0
    for label, launches, make in cases:
        (f0, o0), (f1, o1) = (make(lib) for lib in libs)
        f0(), f1()
        torch.cuda.synchronize()
        same = all(torch.equal(a, b) for a, b in zip(o0, o1))
        (a, b) = windows([f0, f1], launches)
        worst = max(worst, b[0] / a[0])
        say('| %s | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %.3f | %s | %s |' % ((label,) + a + b + (b[0] / a[0], b[0] / a[0] <= BAR, same)))
        del f0, f1, o0, o1
        torch.cuda.empty_cache()
    say()
    say('Largest ratio: %.3f.' % worst)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

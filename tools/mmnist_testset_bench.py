"""Time of the Moving-MNIST test set on the device at the reference's size (10 000 stand-in digits -> 5 000 videos of 100 frames of 64 x 64,
seed 42): the one vs_moving_mnist_testset launch as uint8 (the file's layout) and as fp32 (the layout kept in HBM); the same videos through
the training renderer (ops.moving_mnist_batch: normalised fp32, the same kernel body and at this size the same one workgroup per video);
the fill rate of buffers of the outputs' sizes (what the frame stores alone could cost); the NumPy restatement of the same set (tests/mmnist_testset_ref.py) on the host; and the
stages of the command line (preprocessing/mnist/make_test_set.py), np.savez_compressed among them.  Every device time is the median over
REPS windows of LAUNCHES launches between two events, warm.  Writes the note given by --out (default profiles/mmnist_testset_timing.md).

    python tools/mmnist_testset_bench.py [--out FILE] [--host-videos N]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import mmnist_testset_inputs as I  # noqa: E402
import mmnist_testset_ref as R  # noqa: E402
from spatiotemporal_variable_separation_amd import _lib, ops  # noqa: E402
from spatiotemporal_variable_separation_amd.data.moving_mnist import draw_test_set, synthetic_digits  # noqa: E402
from spatiotemporal_variable_separation_amd.preprocessing.mnist import make_test_set  # noqa: E402

N_IMAGES, T, F, ND, SPEED, SEED = 10000, 100, 64, 2, 4, 42
REPS, LAUNCHES = 7, 10


def windows_ms(fn):
    """(median, min, max) ms per launch over REPS windows of LAUNCHES launches."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / LAUNCHES)
    return float(np.median(ts)), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mmnist_testset_timing.md'))
    ap.add_argument('--host-videos', type=int, default=5000, help='videos of the set that the NumPy restatement renders (scaled to 5 000)')
    args = ap.parse_args()
    lib = _lib.load_library()
    dev = torch.device('cuda', 0)
    images = synthetic_digits(N_IMAGES, seed=SEED)
    labels = (np.arange(N_IMAGES) % 10).astype(np.uint8)
    _, init = draw_test_set(N_IMAGES, images.shape[1:], F, SPEED, ND, SEED)
    V = init.shape[0]
    d_img, d_init = torch.from_numpy(images).to(dev), torch.from_numpy(init).to(dev)
    u8 = torch.empty((T, V, 1, F, F), dtype=torch.uint8, device=dev)
    f32 = torch.empty((V, T, 1, F, F), dtype=torch.float32, device=dev)
    old, made = torch.empty((V, T, 1, F, F), dtype=torch.float32, device=dev), {}     # `old`: a buffer of the batch's size for the fill
    lat = torch.empty((T, V, ND, 4), dtype=torch.int32, device=dev)

    def testset(out, fp32, st, sv):
        _lib.check(lib.vs_moving_mnist_testset(d_img.data_ptr(), N_IMAGES, 28, 28, d_init.data_ptr(), V, ND, T, F, out.data_ptr(), fp32, st, sv,
                                               lat.data_ptr(), _lib.stream_ptr()), 'vs_moving_mnist_testset')

    def batch():
        made['batch'] = ops.moving_mnist_batch(d_img, d_init, T, F)

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rows = [('vs_moving_mnist_testset, uint8 [T, N, 1, F, F]', lambda: testset(u8, 0, V * F * F, F * F), u8),
            ('vs_moving_mnist_testset, fp32 [N, T, 1, F, F]', lambda: testset(f32, 1, F * F, T * F * F), f32),
            ('vs_moving_mnist_batch, fp32 / 255 [N, T, 1, F, F] (the training renderer)', batch, old)]
    say('# The Moving-MNIST test set at the reference\'s size (one MI355X, `tools/mmnist_testset_bench.py`)')
    say('')
    say('%d stand-in digits -> %d videos x %d frames of %d x %d, %d digits, speed %d, seed %d.  Median (min - max) per launch over %d windows '
        'of %d launches between two events, warm.' % (N_IMAGES, V, T, F, F, ND, SPEED, SEED, REPS, LAUNCHES))
    say('')
    say('| launch | output | time per launch | stores | fill of the same size |')
    say('|---|---|---|---|---|')
    times = {}
    for name, fn, out in rows:
        ms = windows_ms(fn)
        nbytes = out.numel() * out.element_size()
        fill = windows_ms(lambda: out.view(torch.uint8).fill_(7))
        times[name] = ms[0]
        say('| %s | %.3f GB | %.3f ms (%.3f - %.3f) | %.2f TB/s | %.3f ms = %.2f TB/s |'
            % (name, nbytes / 1e9, ms[0], ms[1], ms[2], nbytes / ms[0] / 1e9, fill[0], nbytes / fill[0] / 1e9))
        fn()                                                              # the fill overwrote the frames
    torch.cuda.synchronize()
    same = bool(torch.equal(made['batch'], f32.div(torch.tensor(255., device=dev)))) and bool(torch.equal(f32, u8.transpose(0, 1).float()))
    say('')
    say('* The three outputs describe the same videos (fp32 = uint8, training renderer = fp32 / 255 bit for bit): %s.' % same)
    names = [r[0] for r in rows]
    say('* Raw against normalised fp32 (same bytes written, same launch shape here): %.3f ms against %.3f ms = %.2f x.'
        % (times[names[1]], times[names[2]], times[names[2]] / times[names[1]]))

    n_host = min(args.host_videos, V)
    t0 = time.perf_counter()
    seq, _ = R.render(images, init[:n_host], T, F)
    host_s = (time.perf_counter() - t0) * V / n_host
    say('* NumPy restatement (`tests/mmnist_testset_ref.py`) on the same box\'s host: %.1f s for the set (%d videos rendered%s) = %.0f x the '
        'uint8 launch.' % (host_s, n_host, '' if n_host == V else ', scaled', host_s * 1e3 / times[names[0]]))
    say('* Its first %d videos equal the launch\'s: %s.' % (n_host, bool(np.array_equal(seq, u8[:, :n_host].cpu().numpy()))))

    with tempfile.TemporaryDirectory() as tmp:
        I.write_t10k(tmp, images, labels)
        stages = {}
        t0 = time.perf_counter()
        arrays = make_test_set.generate(tmp, T, SEED, ND, F, SPEED, dev, timings=stages)
        t1 = time.perf_counter()
        path = os.path.join(tmp, 'mmnist_test_2digits_64.npz')
        np.savez_compressed(path, **arrays)
        t2 = time.perf_counter()
        total = t2 - t0
        say('* The command line, %.1f s in all: read %.2f s, draws %.2f s, launch %.4f s, download %.2f s, `np.savez_compressed` %.1f s = '
            '%.0f %% (file of %.1f MB).' % (total, stages['read'], stages['draw'], stages['kernel'], stages['download'], t2 - t1,
                                            100 * (t2 - t1) / total, os.path.getsize(path) / 1e6))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

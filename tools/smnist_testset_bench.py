"""Time of the STOCHASTIC Moving-MNIST test set on the device at the reference's size (10 000 stand-in digits -> 5 000 videos of 100 frames
of 64 x 64, 2 digits, speed 4, seed 42):
  1. the walk launch (vs_mmnist_stochastic_trajectories: 10 000 trajectories of 100 frames, four prefix draws, latents, ONE workgroup) from
     the stream as the permutation leaves it; consecutive launches continue the stream, so every launch walks other trajectories of the same kind;
  2. the render launch (vs_moving_mnist_testset_place) as uint8 time-major and as fp32 video-major, in the same process and in alternating
     windows with vs_moving_mnist_testset (which also walks its deterministic trajectories) at the same size; the bar is 1.10 x;
  3. the host loop (the four draws and `_stochastic_collision` of data/moving_mnist.py, what `MovingMNIST.draw_stochastic` runs per digit)
     on the same box, on the first --host-videos videos, scaled, and compared with the launch's latents;
  4. the whole command `make_test_set --stochastic` in a fresh process, with VARSEP_NPZ_COMPRESS=host and =device.
Device times are medians over REPS windows between two events, warm.  Writes the note given by --out (default
profiles/smnist_testset_timing.md); the code-object figures of the walk kernel are in that note by hand (they come from the compiler).

    python tools/smnist_testset_bench.py [--out FILE] [--host-videos N] [--skip-cli]
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import mmnist_testset_inputs as I  # noqa: E402
from spatiotemporal_variable_separation_amd import _lib  # noqa: E402
from spatiotemporal_variable_separation_amd.data import moving_mnist as M  # noqa: E402
from spatiotemporal_variable_separation_amd.data.numpy_stream import DeviceRandomState  # noqa: E402

N_IMAGES, T, F, ND, SPEED, SEED = 10000, 100, 64, 2, 4, 42
REPS, LAUNCHES, WALKS = 7, 10, 3
ROOM = F - 28


def window_ms(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def windows_ms(fn, launches=LAUNCHES):
    """(median, min, max) ms per launch over REPS windows of `launches` launches."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = [window_ms(fn, launches) for _ in range(REPS)]
    return float(np.median(ts)), min(ts), max(ts)


def alternating_ms(fa, fb):
    """((median, min, max) of fa, the same of fb): REPS pairs of windows, a window of fa then a window of fb."""
    for _ in range(3):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REPS):
        ta.append(window_ms(fa, LAUNCHES))
        tb.append(window_ms(fb, LAUNCHES))
    return (float(np.median(ta)), min(ta), max(ta)), (float(np.median(tb)), min(tb), max(tb))


def host_walk(n_videos):
    """latents [T, n_videos, ND, 4] from the GLOBAL stream as it stands: the host loop of the stochastic sampler, four draws per digit."""
    rnd = np.random.randint
    lat = np.empty((T, n_videos, ND, 4), dtype=np.int32)
    for v in range(n_videos):
        for n in range(ND):
            sx, sy = rnd(0, ROOM + 1), rnd(0, ROOM + 1)
            dx, dy = rnd(-SPEED, SPEED + 1), rnd(-SPEED, SPEED + 1)
            for t in range(T):
                sx, sy, dx, dy = M._stochastic_collision(rnd, sx, sy, dx, dy, ROOM, ROOM, SPEED)
                lat[t, v, n] = (int(round(sx)), int(round(sy)), dx, dy)
                sy += dy
                sx += dx
    return lat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'smnist_testset_timing.md'))
    ap.add_argument('--host-videos', type=int, default=5000, help='videos whose trajectories the host loop walks (scaled to 5 000)')
    ap.add_argument('--skip-cli', action='store_true', help='leave out the two runs of the whole command')
    args = ap.parse_args()
    lib = _lib.load_library()
    dev = torch.device('cuda', 0)
    images = M.synthetic_digits(N_IMAGES, seed=SEED)
    labels = (np.arange(N_IMAGES) % 10).astype(np.uint8)
    d_img = torch.from_numpy(images).to(dev)
    V = N_IMAGES // ND
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# The stochastic Moving-MNIST test set at the reference\'s size (one MI355X, `tools/smnist_testset_bench.py`)')
    say('')
    say('%d stand-in digits -> %d videos x %d frames of %d x %d, %d digits, speed %d, seed %d.  Median (min - max) per launch over %d windows '
        'between two events, warm.' % (N_IMAGES, V, T, F, F, ND, SPEED, SEED, REPS))
    say('')

    # ---- the set itself, once, validated: what the launches below write again
    digits_idx, frames, latents = M.stochastic_test_set(d_img, F, SPEED, ND, SEED, T)
    after_set = np.random.get_state()
    positions = latents[..., :2].contiguous()
    idx = torch.from_numpy(digits_idx[:V * ND].astype(np.int32)).to(dev).view(V, ND)

    # ---- 1. the walk
    np.random.seed(SEED)
    np.random.permutation(N_IMAGES)
    after_permutation = np.random.get_state()
    rs = DeviceRandomState(None, dev)
    cols = ((0, 0, -SPEED, -SPEED), (ROOM + 1, ROOM + 1, SPEED + 1, SPEED + 1))

    def walk():
        rs.stochastic_trajectories(V * ND, T, cols[0], cols[1], ROOM, ROOM, SPEED, latents=True)

    first = rs.stochastic_trajectories(V * ND, T, cols[0], cols[1], ROOM, ROOM, SPEED, latents=True)[2]
    same_walk = bool(torch.equal(first.view(T, V, ND, 4), latents))
    rs = DeviceRandomState(None, dev)
    walk_ms = windows_ms(walk, WALKS)
    say('| launch | time per launch |')
    say('|---|---|')
    say('| `vs_mmnist_stochastic_trajectories`, %d trajectories x %d frames, four prefix draws, latents (one workgroup) | **%.2f ms** (%.2f - %.2f), '
        'windows of %d launches that continue the stream |' % (V * ND, T, walk_ms[0], walk_ms[1], walk_ms[2], WALKS))

    # ---- 2. the renderer beside vs_moving_mnist_testset
    np.random.set_state(after_permutation)
    _, init = M.draw_test_set(N_IMAGES, images.shape[1:], F, SPEED, ND, SEED)
    d_init = torch.from_numpy(init).to(dev)
    u8 = torch.empty((T, V, 1, F, F), dtype=torch.uint8, device=dev)
    f32 = torch.empty((V, T, 1, F, F), dtype=torch.float32, device=dev)
    lat = torch.empty((T, V, ND, 4), dtype=torch.int32, device=dev)

    def place(out, fp32, st, sv):
        _lib.check(lib.vs_moving_mnist_testset_place(d_img.data_ptr(), N_IMAGES, 28, 28, positions.data_ptr(), idx.data_ptr(), V, ND, T, F,
                                                     out.data_ptr(), fp32, st, sv, None, _lib.stream_ptr()), 'vs_moving_mnist_testset_place')

    def testset(out, fp32, st, sv):
        _lib.check(lib.vs_moving_mnist_testset(d_img.data_ptr(), N_IMAGES, 28, 28, d_init.data_ptr(), V, ND, T, F, out.data_ptr(), fp32, st, sv,
                                               lat.data_ptr(), _lib.stream_ptr()), 'vs_moving_mnist_testset')

    ratios, place_ms = {}, {}
    for tag, out, fp32, st, sv in (('uint8 [T, N, 1, F, F]', u8, 0, V * F * F, F * F), ('fp32 [N, T, 1, F, F]', f32, 1, F * F, T * F * F)):
        mine, theirs = alternating_ms(lambda: place(out, fp32, st, sv), lambda: testset(out, fp32, st, sv))
        nbytes = out.numel() * out.element_size()
        ratios[tag], place_ms[tag] = mine[0] / theirs[0], mine[0]
        say('| `vs_moving_mnist_testset_place`, %s | %.3f ms (%.3f - %.3f) = %.2f TB/s of stores |' % (tag, mine[0], mine[1], mine[2], nbytes / mine[0] / 1e9))
        say('| `vs_moving_mnist_testset`, %s, alternating windows of %d launches | %.3f ms (%.3f - %.3f); the new launch is **%.3f x** this |'
            % (tag, LAUNCHES, theirs[0], theirs[1], theirs[2], ratios[tag]))
        place(out, fp32, st, sv)
    torch.cuda.synchronize()
    same = bool(torch.equal(u8, frames)) and bool(torch.equal(f32, u8.transpose(0, 1).float()))
    say('')
    say('* The renderer against the bar of 1.10 x `vs_moving_mnist_testset` in the same run: %s.'
        % ', '.join('%s %.3f x (%s)' % (k, v, 'within' if v <= 1.10 else 'OVER') for k, v in ratios.items()))
    say('* The timed launches wrote the set that `stochastic_test_set` made (uint8 = fp32, walk = the set\'s latents): %s.' % (same and same_walk))
    both = walk_ms[0] + place_ms['uint8 [T, N, 1, F, F]']
    say('* Walk + uint8 render: %.2f ms for the set; the walk is %.0f %% of it.' % (both, 100 * walk_ms[0] / both))

    # ---- 3. the host loop
    n_host = min(args.host_videos, V)
    np.random.set_state(after_permutation)
    t0 = time.perf_counter()
    host_lat = host_walk(n_host)
    host_s = (time.perf_counter() - t0) * V / n_host
    say('* The host loop (four draws and `_stochastic_collision` per step, Python) on the same box: %.2f s for the set (%d videos walked%s) = '
        '**%.0f x** the walk launch.' % (host_s, n_host, '' if n_host == V else ', scaled', host_s * 1e3 / walk_ms[0]))
    say('* Its latents equal the launch\'s: %s.' % bool(np.array_equal(host_lat, latents[:, :n_host].cpu().numpy())))
    np.random.set_state(after_set)

    # ---- 4. the whole command, a fresh process each
    if not args.skip_cli:
        with tempfile.TemporaryDirectory() as tmp:
            I.write_t10k(tmp, images, labels)
            for compress in ('host', 'device'):
                cmd = [sys.executable, '-m', 'spatiotemporal_variable_separation_amd.preprocessing.mnist.make_test_set', '--data_dir', tmp, '--device',
                       '0', '--stochastic']
                t0 = time.perf_counter()
                r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, VARSEP_NPZ_COMPRESS=compress), capture_output=True, text=True, timeout=600)
                secs = time.perf_counter() - t0
                path = os.path.join(tmp, 'smmnist_test_2digits_64.npz')
                if r.returncode != 0:
                    say('* `make_test_set --stochastic`, VARSEP_NPZ_COMPRESS=%s: FAILED (%d) %s' % (compress, r.returncode, r.stderr[-400:]))
                    continue
                with np.load(path) as z:
                    ok = bool(np.array_equal(z['latents'], latents.cpu().numpy())) and bool(np.array_equal(z['sequences'][:, :50], frames[:, :50].cpu().numpy()))
                say('* `make_test_set --stochastic`, VARSEP_NPZ_COMPRESS=%s, a fresh process (imports and device start-up included): %.1f s, file of '
                    '%.1f MB, its latents and first 50 videos equal the set above: %s.' % (compress, secs, os.path.getsize(path) / 1e6, ok))
                os.remove(path)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

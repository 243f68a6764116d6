"""Time and size of the Moving-MNIST evaluation command's result files on both routes of VARSEP_NPZ_COMPRESS, at the paper's setting (5 000
test videos, nt_cond 5, --nt_pred 95, 64 x 64 x 1, batch 16: 8.09 GB of uint8 frames in six files).  No trained checkpoint is needed: a
freshly initialised DCGAN model of the paper's shapes (configs.BASELINE_CONFIGS['mnist_b16']) is saved once, the test set is generated in
HBM from stand-in idx files (`--data_dir generated:D`, seeded digit-like blobs as tools/deflate_bench.py uses), and `main` of
test/mnist/test.py runs with `host` and `device` alternating, twice each, every run in a fresh child process.  Per run: the wall time of
the command (the child process from start to exit) and of `main`, the time inside the save calls (the device is synchronised before each,
so that pending forecast work is not counted as saving), the bytes written, and for predictions.npz the size of the device-written file
against the host-written one.  An untrained model's forecasts are not a trained model's, which are smoother.  Writes the note given by
--out.

    python tools/eval_npz_bench.py [--out FILE] [--videos N] [--nt_pred P] [--batch_size B] [--tmp DIR]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

CONFIG = 'mnist_b16'
N_TRAIN, ND, SEED = 1000, 2, 42
FILES = ['results.npz', 'predictions.npz', 'gt.npz', 'cond.npz', 'content_swap.npz', 'cond_swap.npz', 'target_swap.npz']
ORDER = ('host', 'device', 'host', 'device')               # alternating; every run is reported


def child(args):
    """One run of the command's `main` in this (fresh) process; prints one JSON line."""
    os.environ['VARSEP_NPZ_COMPRESS'] = args.child
    import torch
    from spatiotemporal_variable_separation_amd.test.mnist import test as cli
    from spatiotemporal_variable_separation_amd.utils import savez
    saves = []
    inner = savez.savez_compressed

    def timed(path, arrays, *a, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        inner(path, arrays, *a, **kw)
        saves.append((os.path.basename(path), time.perf_counter() - t0))

    savez.savez_compressed = timed
    argv = ['--xp_dir', args.xp_dir, '--data_dir', 'generated:' + args.data_dir, '--nt_pred', str(args.nt_pred),
            '--batch_size', str(args.batch_size), '--device', '0']
    t0 = time.perf_counter()
    cli.main(cli.build_parser(stochastic=True).parse_args(argv))
    main_s = time.perf_counter() - t0
    print('EVAL_NPZ_BENCH ' + json.dumps(dict(route=args.child, main_s=main_s, saves=saves, peak_hbm=torch.cuda.max_memory_allocated())), flush=True)


def write_inputs(tmp, videos):
    """The stand-in idx files under tmp/data and the untrained model with its params.json under tmp/xp."""
    import torch
    import mmnist_testset_inputs as I
    from spatiotemporal_variable_separation_amd.configs import BASELINE_CONFIGS
    from spatiotemporal_variable_separation_amd.data.moving_mnist import synthetic_digits
    from spatiotemporal_variable_separation_amd.networks.factory import build_sep_net
    from spatiotemporal_variable_separation_amd.utils.helper import save
    data, xp = os.path.join(tmp, 'data'), os.path.join(tmp, 'xp')
    n_images = videos * ND
    I.write_t10k(data, synthetic_digits(n_images, seed=SEED), (np.arange(n_images) % 10).astype(np.uint8))
    train = synthetic_digits(N_TRAIN, seed=SEED + 1)
    with open(os.path.join(data, 'MNIST', 'raw', 'train-images-idx3-ubyte'), 'wb') as f:
        f.write(np.array([2051, N_TRAIN, 28, 28], dtype='>i4').tobytes() + train.tobytes())
    cfg = BASELINE_CONFIGS[CONFIG]
    torch.manual_seed(SEED)
    save(xp, build_sep_net(cfg))
    with open(os.path.join(xp, 'params.json'), 'w') as f:
        json.dump(dict(architecture=cfg['architecture'], data='mnist', n_object=ND, nt_cond=cfg['nt_cond'], nt_pred=cfg['nt_pred'],
                       offset=cfg['offset'], skipco=cfg['skipco']), f, indent=4, sort_keys=True)
    return data, xp


def members(path):
    """[(name, uncompressed bytes, CRC-32)] of a zip file's directory."""
    with zipfile.ZipFile(path) as z:
        return [(i.filename, i.file_size, i.CRC) for i in z.infolist()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_npz_timing.md'))
    ap.add_argument('--videos', type=int, default=5000, help='test videos (the paper: 5 000)')
    ap.add_argument('--nt_pred', type=int, default=95)
    ap.add_argument('--batch_size', type=int, default=16)
    ap.add_argument('--tmp', default=None, help='directory for the inputs and the result files of one run at a time (default: the system\'s)')
    ap.add_argument('--child', choices=['host', 'device'], default=None, help=argparse.SUPPRESS)
    ap.add_argument('--xp_dir', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--data_dir', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    nt_cond = 5
    frames = args.videos * (3 * args.nt_pred + (nt_cond + args.nt_pred) + 2 * nt_cond)
    say('# The Moving-MNIST evaluation command\'s result files on both routes of VARSEP_NPZ_COMPRESS (one MI355X, `tools/eval_npz_bench.py`)')
    say()
    say('`test.mnist.test --data_dir generated:D --nt_pred %d --batch_size %d` on %d test videos (nt_cond %d, 64 x 64 x 1): %d uint8 frames = '
        '%.3f GB in six files, plus the small float file results.npz.  The model is a freshly initialised DCGAN network of the paper\'s shapes '
        '(`%s`), the digits are seeded stand-in blobs.  **An untrained model\'s forecasts are not a trained model\'s, which are smoother**: '
        'the sizes of predictions.npz and content_swap.npz below are those of an untrained model\'s output, the sizes of the four data '
        'files (gt, cond, cond_swap, target_swap) do not depend on the model.' % (args.nt_pred, args.batch_size, args.videos, nt_cond, frames,
                                                                                  frames * 4096 / 1e9, CONFIG))
    say()
    say('Every run is a fresh child process; the routes alternate; every run is reported.  Wall times, one run each, same box, same '
        'session.  "command": the child process from start to exit (interpreter start, imports, data generation, model load, forecasts, '
        'files).  "main": inside `main`.  "save calls": inside the seven `savez_compressed` calls, the device synchronised before each.  '
        'The host route also downloads six uint8 arrays per batch during the loop (%d batches); that time is in "main", not in "save calls".'
        % (-(-args.videos // args.batch_size)))
    say()
    runs = []
    with tempfile.TemporaryDirectory(dir=args.tmp) as tmp:
        data, xp_template = write_inputs(tmp, args.videos)
        say('| run | route | command | main | save calls | bytes written | predictions.npz | peak HBM (torch allocator) |')
        say('|---|---|---|---|---|---|---|---|')
        for k, route in enumerate(ORDER):
            xp = os.path.join(tmp, 'run')
            shutil.copytree(xp_template, xp)
            t0 = time.perf_counter()
            p = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--child', route, '--xp_dir', xp, '--data_dir', data,
                                  '--nt_pred', str(args.nt_pred), '--batch_size', str(args.batch_size)], cwd=ROOT, stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, text=True)
            while True:
                try:
                    stdout, stderr = p.communicate(timeout=60)
                    break
                except subprocess.TimeoutExpired:
                    print('  (the %s run is at %d s)' % (route, time.perf_counter() - t0), flush=True)
            wall = time.perf_counter() - t0
            if p.returncode != 0:
                sys.exit('the %s run failed (exit %d):\n%s\n%s' % (route, p.returncode, stdout[-2000:], stderr[-4000:]))
            rec = json.loads([ln for ln in stdout.splitlines() if ln.startswith('EVAL_NPZ_BENCH ')][-1].split(' ', 1)[1])
            rec.update(wall=wall, sizes={n: os.path.getsize(os.path.join(xp, n)) for n in FILES}, members={n: members(os.path.join(xp, n)) for n in FILES})
            rec['save_s'] = sum(s for _, s in rec['saves'])
            assert [n for n, _ in rec['saves']] == FILES, rec['saves']
            runs.append(rec)
            say('| %d | VARSEP_NPZ_COMPRESS=%s | %.2f s | %.2f s | **%.2f s** | %.1f MB | %.1f MB | %.2f GB |'
                % (k + 1, route, wall, rec['main_s'], rec['save_s'], sum(rec['sizes'].values()) / 1e6, rec['sizes']['predictions.npz'] / 1e6,
                   rec['peak_hbm'] / 1e9))
            shutil.rmtree(xp)
    say()
    host, device = [r for r in runs if r['route'] == 'host'], [r for r in runs if r['route'] == 'device']
    say('## Per file (first run of each route)')
    say()
    say('| file | uncompressed | host: bytes | host: seconds | device: bytes | device: seconds | device / host bytes |')
    say('|---|---|---|---|---|---|---|')
    for n in FILES:
        h, d = host[0], device[0]
        raw = sum(u for _, u, _ in h['members'][n])
        say('| %s | %.1f MB | %d | %.2f | %d | %.2f | %.3f |' % (n, raw / 1e6, h['sizes'][n], dict(h['saves'])[n], d['sizes'][n], dict(d['saves'])[n],
                                                                 d['sizes'][n] / h['sizes'][n]))
    say()
    same = all(r['members'] == runs[0]['members'] for r in runs)
    ratio = device[0]['sizes']['predictions.npz'] / host[0]['sizes']['predictions.npz']
    med = lambda rs, key: float(np.median([r[key] for r in rs]))  # noqa: E731
    say('* Member names, uncompressed sizes and CRC-32s (over the .npy header and the data) of all seven files are %s in all four runs.'
        % ('equal' if same else '**NOT equal**'))
    say('* predictions.npz, device-written against host-written: **%.3f x** (%d against %d bytes)%s.'
        % (ratio, device[0]['sizes']['predictions.npz'], host[0]['sizes']['predictions.npz'],
           ' -- above 1.25 x' if ratio > 1.25 else ''))
    say('* The four data files are video-major, [N, T, 64, 64, 1]: consecutive frames of one video lie 4096 bytes apart and differ by a shift '
        'of the digits, which zlib\'s window search finds and the device encoder (runs at distance 1, independent 32 KiB chunks) does not: '
        'gt.npz is **%.2f x** and target_swap.npz **%.2f x** the host-written size.  (The test-set file of profiles/deflate_timing.md is '
        'time-major, [T, N, ...]: neighbouring frames belong to different videos, and there the encoder reached 0.992 x.  Host zlib on 64 '
        'stand-in videos of 100 frames, `Z_RLE` on independent 32 KiB chunks against level 6 over the whole stream: 4.94 x video-major, '
        '0.99 x time-major.)  A trained model\'s forecasts look more like these data frames than an untrained model\'s do, so its '
        'predictions.npz and content_swap.npz must be expected nearer to the data files\' ratio than to the one measured here.'
        % (device[0]['sizes']['gt.npz'] / host[0]['sizes']['gt.npz'], device[0]['sizes']['target_swap.npz'] / host[0]['sizes']['target_swap.npz']))
    say('* All files: %.1f MB device-written against %.1f MB host-written (%.3f x).'
        % (sum(device[0]['sizes'].values()) / 1e6, sum(host[0]['sizes'].values()) / 1e6, sum(device[0]['sizes'].values()) / sum(host[0]['sizes'].values())))
    say('* Save calls: %.2f s (host) against %.2f s (device); `main`: %.2f s against %.2f s; the command: %.2f s against %.2f s (means of the '
        'two runs of each route).' % (med(host, 'save_s'), med(device, 'save_s'), med(host, 'main_s'), med(device, 'main_s'), med(host, 'wall'),
                                      med(device, 'wall')))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

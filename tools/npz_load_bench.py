"""Time and memory of reading the Moving-MNIST test-set file on the device (utils/loadz.py, csrc/vs_inflate_chunks.hip) at the reference's
size (10 000 stand-in digits -> 5 000 videos of 100 frames of 64 x 64, as tools/deflate_bench.py builds them), on the file written three
ways: VARSEP_NPZ_COMPRESS=device with VARSEP_NPZ_MATCH=runs, the same with =window, and np.savez_compressed.  Per file: the launches of
ops.inflate_raw on the `sequences` member by kernel (event times, one warm pass), and the whole `MovingMNIST.make_dataset(train=False)`
with VARSEP_NPZ_LOAD=device and =host, alternating, every run in a fresh process, with the peak of HBM torch allocated.  The comparison
is the host route on the same box in the same run.  Writes the note given by --out.

    python tools/npz_load_bench.py [--out FILE] [--videos N] [--pairs K]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from spatiotemporal_variable_separation_amd import ops  # noqa: E402
from spatiotemporal_variable_separation_amd.data.moving_mnist import MovingMNIST, synthetic_digits  # noqa: E402
from spatiotemporal_variable_separation_amd.utils import npz, savez  # noqa: E402

N_IMAGES, T, F, ND, SPEED, SEED = 10000, 100, 64, 2, 4, 42
NAME = 'mmnist_test_%ddigits_%d.npz' % (ND, F)
KERNELS = ('vs_inflate_sync_scan', 'vs_inflate_segments', 'vs_inflate_place', 'vs_inflate_resolve', 'vs_crc32')

lines = []


def say(s=''):
    print(s, flush=True)
    lines.append(s)


def child(directory, route):
    """One make_dataset(train=False) in this (fresh) process: a JSON line with the seconds, the peak HBM and a checksum of .data."""
    dev = torch.device('cuda', 0)
    torch.zeros(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    report = {}
    t0 = time.perf_counter()
    ds = MovingMNIST.make_dataset(directory, F, 5, 10, SPEED, True, ND, False, device=dev, load=route, report=report)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print(json.dumps(dict(seconds=seconds, peak=torch.cuda.max_memory_allocated(dev), shape=list(ds.data.shape),
                          checksum=float(ds.data.sum(dtype=torch.float64).item()), report={k: list(v) for k, v in report.items()})))


def run_child(directory, route):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', directory, route], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('child %s %s failed (%d):\n%s' % (directory, route, r.returncode, r.stderr[-3000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def kernel_table(label, path, dev):
    entry = {e.name: e for e in npz.read_directory(path)}['sequences.npy']
    t0 = time.perf_counter()
    comp = torch.from_numpy(np.fromfile(path, dtype=np.uint8, count=entry.csize, offset=entry.data_offset)).to(dev)
    torch.cuda.synchronize()
    upload = time.perf_counter() - t0
    out = ops.inflate_raw(comp, entry.usize, crc=entry.crc32)               # warm
    chained = isinstance(out, torch.Tensor)
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    ops.profile_reset(True)
    t0 = time.perf_counter()
    out = ops.inflate_raw(comp, entry.usize, crc=entry.crc32)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    prof = ops.profile_collect()
    peak = torch.cuda.max_memory_allocated(dev) - base
    say('## %s: `sequences` is %d compressed bytes (%.1f MB) for %d (%.3f GB)' % (label, entry.csize, entry.csize / 1e6, entry.usize, entry.usize / 1e9))
    say()
    if not chained:
        say('* ops.inflate_raw: %r after %.3f s (scan %.3f ms in %d launches, segments %.3f ms): the member takes the host route.'
            % (out, wall, prof.get('vs_inflate_sync_scan', {}).get('ms', 0.0), prof.get('vs_inflate_sync_scan', {}).get('n', 0),
               prof.get('vs_inflate_segments', {}).get('ms', 0.0)))
        say()
        return
    say('| launch | launches | event time, summed | output bytes per second of it |')
    say('|---|---|---|---|')
    for k in KERNELS:
        p = prof.get(k, {'ms': 0.0, 'n': 0})
        whole = p['ms'] and k != 'vs_inflate_resolve'                        # (resolve touches the segments with external bytes only)
        say('| %s | %d | %.3f ms | %s |' % (k, p['n'], p['ms'], '%.1f GB/s' % (entry.usize / p['ms'] / 1e6) if whole else '-'))
    total = sum(prof.get(k, {'ms': 0.0})['ms'] for k in KERNELS)
    say('| all launches | %d | %.3f ms | %.1f GB/s |' % (sum(prof.get(k, {'n': 0})['n'] for k in KERNELS), total, entry.usize / total / 1e6))
    say()
    say('* ops.inflate_raw, wall clock with its downloads of the report words and the chain walk on the host: %.3f s; reading the member from '
        'the file and uploading it: %.3f s; HBM allocated above the compressed bytes, at the peak: %.2f GB (the output is %.2f GB).'
        % (wall, upload, peak / 1e9, entry.usize / 1e9))
    say()
    del out, comp
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'npz_load_timing.md'))
    ap.add_argument('--videos', type=int, default=N_IMAGES // ND, help='videos of the set (the reference: 5 000)')
    ap.add_argument('--pairs', type=int, default=2, help='(device, host) pairs of fresh processes per file')
    ap.add_argument('--child', nargs=2, metavar=('DIR', 'ROUTE'), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    import mmnist_testset_inputs as I
    from spatiotemporal_variable_separation_amd.preprocessing.mnist import make_test_set
    dev = torch.device('cuda', 0)
    n_images = args.videos * ND
    images = synthetic_digits(n_images, seed=SEED)
    labels = (np.arange(n_images) % 10).astype(np.uint8)
    say('# Reading the Moving-MNIST test-set file on the device (one MI355X, `tools/npz_load_bench.py`)')
    say()
    say('%d videos x %d frames of %d x %d.  Kernel times are HIP event times of one warm pass; everything else is wall clock on the same box in '
        'the same run, one fresh process per `make_dataset`.' % (args.videos, T, F, F))
    say()
    with tempfile.TemporaryDirectory() as tmp:
        I.write_t10k(tmp, images, labels)
        arrays = make_test_set.generate_device(tmp, T, SEED, ND, F, SPEED, dev)
        files = []
        for label, compress, match in (('device writer, runs matcher', 'device', 'runs'), ('device writer, window matcher', 'device', 'window'),
                                       ('np.savez_compressed', 'host', None)):
            d = os.path.join(tmp, (match or 'numpy'))
            os.makedirs(d)
            t0 = time.perf_counter()
            savez.savez_compressed(os.path.join(d, NAME), arrays, compress=compress, match=match)
            files.append((label, d, time.perf_counter() - t0))
        del arrays
        torch.cuda.empty_cache()
        say('| file | written in | size |')
        say('|---|---|---|')
        for label, d, s in files:
            say('| %s | %.2f s | %.1f MB |' % (label, s, os.path.getsize(os.path.join(d, NAME)) / 1e6))
        say()
        for label, d, _ in files:
            kernel_table(label, os.path.join(d, NAME), dev)
        say('## `MovingMNIST.make_dataset(train=False)`, whole, alternating routes, a fresh process each')
        say()
        say('| file | VARSEP_NPZ_LOAD | seconds | peak HBM | `sequences` took | `.data` checksum |')
        say('|---|---|---|---|---|---|')
        for label, d, _ in files:
            for _ in range(args.pairs):
                for route in ('device', 'host'):
                    r = run_child(d, route)
                    took = r['report'].get('sequences', ['host', 'load=host'])
                    say('| %s | %s | **%.2f s** | %.2f GB | %s (%s) | %.0f |' % (label, route, r['seconds'], r['peak'] / 1e9, took[0], took[1], r['checksum']))
        say()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

"""Time and memory of reading the Moving-MNIST test-set file on the device (utils/loadz.py, csrc/vs_inflate_chunks.hip) at the reference's
size (10 000 stand-in digits -> 5 000 videos of 100 frames of 64 x 64, as tools/deflate_bench.py builds them), on the file written three
ways: VARSEP_NPZ_COMPRESS=device with VARSEP_NPZ_MATCH=runs, the same with =window, and np.savez_compressed.  Per file: the launches of
ops.inflate_raw on the `sequences` member by kernel (event times, one warm pass), and the whole `MovingMNIST.make_dataset(train=False)`
with VARSEP_NPZ_LOAD=device and =host, alternating, every run in a fresh process, with the peak of HBM torch allocated.  The comparison
is the host route on the same box in the same run.  Writes the note given by --out.

--blocks: the rule VARSEP_NPZ_FOREIGN on the np.savez_compressed file alone (utils/loadz.npz_foreign, csrc/vs_inflate_blocks.hip): the
launches of ops.inflate_blocks by kernel, the candidates the scan found, the chain's length, the candidates off the chain (each one a false
positive: a chain that verified passes through every block start that is in the list), the scan's misses on a sample of the stream that a
block walker reads on the host, the peak of HBM, and `make_dataset` on the three routes `host`, `device` + foreign `host` (what the file
took before the rule existed) and `device` + foreign `device`, alternating, every run in a fresh process.

--blocks --stored: the rule VARSEP_NPZ_FINDER (utils/loadz.npz_finder, vs_inflate_block_scan_stored) on an np.savez_compressed file of random
uint8 with the test set's shape -- incompressible, so zlib writes stored blocks only: the launches of ops.inflate_blocks(stored=True) by
kernel, the candidates of both finders, how many are on the chain, candidates per true stored block (a block walker on a sample), the
workspace, what the try with the dynamic finder alone costs before it gives up, and utils/loadz.load on the three routes `host`, `device` +
foreign `device` + finder `dynamic` (what the file takes without the stored finder: tried on the device, capped, inflated on the host) and
the same with finder `all`, alternating, every run in a fresh process.  Its note goes BEHIND the --blocks note in the same file (an earlier
note of its own is replaced).

    python tools/npz_load_bench.py [--out FILE] [--videos N] [--pairs K] [--blocks [--stored]] [--sample-mb M]
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
BLOCK_KERNELS = ('vs_inflate_block_scan', 'vs_inflate_block_probe', 'vs_inflate_block_windows', 'vs_inflate_block_decode', 'vs_crc32')
ROUTES = ('host', 'device+host', 'device+device')          # VARSEP_NPZ_LOAD [+ VARSEP_NPZ_FOREIGN]
STORED_TITLE = '# Reading an incompressible NumPy-written .npz member on the device (one MI355X, `tools/npz_load_bench.py --blocks --stored`)'
STORED_KERNELS = BLOCK_KERNELS[:1] + ('vs_inflate_block_scan_stored',) + BLOCK_KERNELS[1:]
STORED_ROUTES = ('host', 'device+device+dynamic', 'device+device+all')   # VARSEP_NPZ_LOAD [+ VARSEP_NPZ_FOREIGN + VARSEP_NPZ_FINDER]

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
    load, _, foreign = route.partition('+')
    t0 = time.perf_counter()
    ds = MovingMNIST.make_dataset(directory, F, 5, 10, SPEED, True, ND, False, device=dev, load=load, report=report, foreign=foreign or None)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print(json.dumps(dict(seconds=seconds, peak=torch.cuda.max_memory_allocated(dev), shape=list(ds.data.shape),
                          checksum=float(ds.data.sum(dtype=torch.float64).item()), report={k: list(v) for k, v in report.items()})))


def child_stored(path, route):
    """One utils/loadz.load of `sequences` in this (fresh) process: a JSON line with the seconds, the peak HBM, a checksum and the route."""
    from spatiotemporal_variable_separation_amd.utils import loadz
    dev = torch.device('cuda', 0)
    torch.zeros(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    report = {}
    load, foreign, finder = (route.split('+') + [None, None])[:3]
    t0 = time.perf_counter()
    got = loadz.load(path, dev, keys=('sequences',), load=load, report=report, foreign=foreign, finder=finder)['sequences']
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print(json.dumps(dict(seconds=seconds, peak=torch.cuda.max_memory_allocated(dev), shape=list(got.shape),
                          checksum=float(got.sum(dtype=torch.int64).item()), report={k: list(v) for k, v in report.items()})))


def run_child(directory, route, flag='--child'):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), flag, directory, route], capture_output=True, text=True)
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


def blocks_table(label, path, dev, sample_mb):
    """ops.inflate_blocks on the `sequences` member of `path`: per-kernel event times of one warm pass, candidates, chain, misses, HBM."""
    import inflate_blocks_inputs as IB
    entry = {e.name: e for e in npz.read_directory(path)}['sequences.npy']
    host_bytes = np.fromfile(path, dtype=np.uint8, count=entry.csize, offset=entry.data_offset)
    t0 = time.perf_counter()
    comp = torch.from_numpy(host_bytes).to(dev)
    torch.cuda.synchronize()
    upload = time.perf_counter() - t0
    say('## %s: `sequences` is %d compressed bytes (%.1f MB) for %d (%.3f GB)' % (label, entry.csize, entry.csize / 1e6, entry.usize, entry.usize / 1e9))
    say()
    first = ops.inflate_raw(comp, entry.usize, crc=entry.crc32)
    say('* ops.inflate_raw (the sync-marker reader, tried first): %r' % (first,))
    out = ops.inflate_blocks(comp, entry.usize, crc=entry.crc32)            # warm
    if not isinstance(out, torch.Tensor):
        say('* ops.inflate_blocks: %r: the member takes the host route.' % (out,))
        say()
        return
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    ops.profile_reset(True)
    trace = []
    t0 = time.perf_counter()
    out = ops.inflate_blocks(comp, entry.usize, crc=entry.crc32, trace=trace)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    prof = ops.profile_collect()
    peak = torch.cuda.max_memory_allocated(dev) - base
    say()
    say('| launch | launches | event time, summed | output bytes per second of it |')
    say('|---|---|---|---|')
    for k in BLOCK_KERNELS:
        p = prof.get(k, {'ms': 0.0, 'n': 0})
        say('| %s | %d | %.3f ms | %s |' % (k, p['n'], p['ms'], '%.1f GB/s' % (entry.usize / p['ms'] / 1e6) if p['ms'] else '-'))
    total = sum(prof.get(k, {'ms': 0.0})['ms'] for k in BLOCK_KERNELS)
    say('| all launches | %d | %.3f ms | %.1f GB/s |' % (sum(prof.get(k, {'n': 0})['n'] for k in BLOCK_KERNELS), total, entry.usize / total / 1e6))
    say()
    summary = trace[-1]
    words = np.concatenate([t['words'] for t in trace[:-1]])
    chain_rows = np.concatenate([np.asarray(t['chain'], dtype=np.int64) + t['first'] for t in trace[:-1]])
    w = words[chain_rows] if len(words) == summary['candidates'] else None
    say('* candidates found by the scan: %d; spans on the chain: %d; candidates off the chain (false positives, decoded and ignored): %d.'
        % (summary['candidates'], summary['chain'], summary['candidates'] - summary['chain']))
    if w is not None:
        bad = words[np.setdiff1d(np.arange(len(words)), chain_rows)]
        say('* spans of the chain: compressed bytes min / median / max %d / %d / %d, bytes produced min / median / max %d / %d / %d; spans with '
            'external bytes: %d, external bytes in all: %d (%.1f %% of the output).'
            % tuple([int(x) for x in (np.min(np.diff(np.append(trace[0]['cand'][chain_rows], w[-1, 1]))) // 8,
                                      np.median(np.diff(np.append(trace[0]['cand'][chain_rows], w[-1, 1]))) // 8,
                                      np.max(np.diff(np.append(trace[0]['cand'][chain_rows], w[-1, 1]))) // 8, w[:, 3].min(), np.median(w[:, 3]), w[:, 3].max(),
                                      (w[:, 4] > 0).sum(), w[:, 4].sum())] + [100.0 * w[:, 4].sum() / max(1, entry.usize)]))
        if len(bad):
            say('* the off-chain probes ended with status ' + ', '.join('%d (%d)' % (s, int((bad[:, 0] == s).sum())) for s in np.unique(bad[:, 0]))
                + '; the longest read %d bytes of input.' % int(((bad[:, 1] - trace[0]['cand'][np.setdiff1d(np.arange(len(words)), chain_rows)]) // 8).max()))
    t0 = time.perf_counter()
    blocks = IB.walk_blocks(host_bytes.tobytes(), stop_bit=8 * int(sample_mb * 1e6))
    walked = time.perf_counter() - t0
    limit = blocks[-1]['end']
    truth = {b['start'] for b in blocks if b['type'] == 2 and not b['final'] and b['start'] > 0}
    cand = {int(c) for c in trace[0]['cand'] if 0 < c < limit}
    kinds = [sum(1 for b in blocks if b['type'] == k) for k in range(3)]
    say('* the scan against a block walker on the host (tests/inflate_blocks_inputs.walk_blocks, %.1f s) over the first %.2f MB of the stream: %d '
        'blocks (%d stored, %d fixed, %d dynamic), %d non-final dynamic block starts, of which the scan MISSED %d; candidates in that range that '
        'are no block start (FALSE POSITIVES): %d.' % (walked, limit / 8e6, len(blocks), kinds[0], kinds[1], kinds[2], len(truth), len(truth - cand),
                                                       len(cand - truth)))
    say('* ops.inflate_blocks, wall clock with its downloads of the report words and the chain walk on the host: %.3f s; reading the member from '
        'the file and uploading it: %.3f s; HBM allocated above the compressed bytes, at the peak: %.2f GB (the output is %.2f GB, the workspace '
        '%.2f GB for batches of %d candidates).' % (wall, upload, peak / 1e9, entry.usize / 1e9, summary['workspace_bytes'] / 1e9, ops.INFLATE_BATCH))
    say()
    del out, comp
    torch.cuda.empty_cache()


def main_blocks(args):
    import mmnist_testset_inputs as I
    from spatiotemporal_variable_separation_amd.preprocessing.mnist import make_test_set
    dev = torch.device('cuda', 0)
    n_images = args.videos * ND
    images = synthetic_digits(n_images, seed=SEED)
    labels = (np.arange(n_images) % 10).astype(np.uint8)
    say('# Reading a NumPy-written Moving-MNIST test-set file on the device (one MI355X, `tools/npz_load_bench.py --blocks`)')
    say()
    say('%d videos x %d frames of %d x %d, written by np.savez_compressed: every member is one zlib stream without sync markers.  Kernel times '
        'are HIP event times of one warm pass; everything else is wall clock on the same box in the same run, one fresh process per '
        '`make_dataset`.' % (args.videos, T, F, F))
    say()
    with tempfile.TemporaryDirectory() as tmp:
        I.write_t10k(tmp, images, labels)
        arrays = make_test_set.generate_device(tmp, T, SEED, ND, F, SPEED, dev)
        d = os.path.join(tmp, 'numpy')
        os.makedirs(d)
        t0 = time.perf_counter()
        savez.savez_compressed(os.path.join(d, NAME), arrays, compress='host', match=None)
        say('The file: %.1f MB, written in %.2f s.' % (os.path.getsize(os.path.join(d, NAME)) / 1e6, time.perf_counter() - t0))
        say()
        del arrays
        torch.cuda.empty_cache()
        blocks_table('np.savez_compressed', os.path.join(d, NAME), dev, args.sample_mb)
        say('## `MovingMNIST.make_dataset(train=False)`, whole, alternating routes, a fresh process each')
        say()
        say('| VARSEP_NPZ_LOAD | VARSEP_NPZ_FOREIGN | seconds | peak HBM | `sequences` took | `.data` checksum |')
        say('|---|---|---|---|---|---|')
        for _ in range(args.pairs):
            for route in ROUTES:
                r = run_child(d, route)
                took = r['report'].get('sequences', ['host', 'load=host'])
                load, _, foreign = route.partition('+')
                say('| %s | %s | **%.2f s** | %.2f GB | %s (%s) | %.0f |' % (load, foreign or '-', r['seconds'], r['peak'] / 1e9, took[0], took[1], r['checksum']))
        say()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def stored_table(path, dev, sample_mb):
    """ops.inflate_blocks(stored=True) on the `sequences` member of `path`: per-kernel event times of one warm pass, the candidates of both
    finders, the chain, candidates per true stored block on a sample, the workspace; and the cost of the try without the stored finder."""
    import inflate_blocks_inputs as IB
    entry = {e.name: e for e in npz.read_directory(path)}['sequences.npy']
    host_bytes = np.fromfile(path, dtype=np.uint8, count=entry.csize, offset=entry.data_offset)
    t0 = time.perf_counter()
    comp = torch.from_numpy(host_bytes).to(dev)
    torch.cuda.synchronize()
    upload = time.perf_counter() - t0
    say('## `sequences` is %d compressed bytes (%.1f MB) for %d (%.3f GB)' % (entry.csize, entry.csize / 1e6, entry.usize, entry.usize / 1e9))
    say()
    for label, kwargs in (('the dynamic finder alone (the default)', {}), ('both finders (stored=True)', dict(stored=True))):
        out = ops.inflate_blocks(comp, entry.usize, crc=entry.crc32, **kwargs)    # warm
        del out
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        ops.profile_reset(True)
        trace = []
        t0 = time.perf_counter()
        out = ops.inflate_blocks(comp, entry.usize, crc=entry.crc32, trace=trace, **kwargs)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        prof = ops.profile_collect()
        peak = torch.cuda.max_memory_allocated(dev) - base
        say('### ops.inflate_blocks with %s: %s after %.3f s of wall clock' % (label, 'the bytes' if isinstance(out, torch.Tensor) else repr(out), wall))
        say()
        say('| launch | launches | event time, summed | bytes per second of it |')
        say('|---|---|---|---|')
        for k in STORED_KERNELS:
            p = prof.get(k, {'ms': 0.0, 'n': 0})
            nbytes = entry.csize * p['n'] if 'scan' in k else entry.usize       # a scan reads the stream once per launch
            say('| %s | %d | %.3f ms | %s |' % (k, p['n'], p['ms'], '%.1f GB/s' % (nbytes / p['ms'] / 1e6) if p['ms'] else '-'))
        total = sum(prof.get(k, {'ms': 0.0})['ms'] for k in STORED_KERNELS)
        say('| all launches | %d | %.3f ms | %.1f GB/s |' % (sum(prof.get(k, {'n': 0})['n'] for k in STORED_KERNELS), total, entry.usize / max(total, 1e-9) / 1e6))
        say()
        say('* HBM allocated above the compressed bytes, at the peak: %.2f GB (the output is %.2f GB).' % (peak / 1e9, entry.usize / 1e9))
        if not isinstance(out, torch.Tensor):
            say()
            continue
        summary = trace[-1]
        say('* candidates: %d, of them %d from the stored finder alone; spans on the chain: %d; candidates off the chain (probed and ignored): %d; '
            'workspace %.2f GB for batches of %d candidates; reading the member from the file and uploading it: %.3f s.'
            % (summary['candidates'], summary['stored_candidates'], summary['chain'], summary['candidates'] - summary['chain'],
               summary['workspace_bytes'] / 1e9, ops.INFLATE_BATCH, upload))
        blocks = IB.walk_blocks(host_bytes[:int(sample_mb * 1e6) + (1 << 17)].tobytes(), stop_bit=8 * int(sample_mb * 1e6))
        limit = blocks[-1]['end']
        truth = {b['start'] for b in blocks if b['type'] == 0 and not b['final'] and b['start'] > 0}
        cand = {int(c) for c in trace[0]['cand'] if 0 < c < limit}
        kinds = [sum(1 for b in blocks if b['type'] == k) for k in range(3)]
        say('* against a block walker on the host over the first %.2f MB of the stream: %d blocks (%d stored, %d fixed, %d dynamic), %d non-final '
            'stored block starts, of which the list MISSES %d; candidates in that range: %d, that is %.2f per true stored block.'
            % (limit / 8e6, len(blocks), kinds[0], kinds[1], kinds[2], len(truth), len(truth - cand), len(cand), len(cand) / max(1, len(truth))))
        say()
        del out
    del comp
    torch.cuda.empty_cache()


def main_stored(args):
    dev = torch.device('cuda', 0)
    say(STORED_TITLE)
    say()
    say('`sequences`: random uint8 [%d, %d, 1, %d, %d] (the shape of the %d x %d test set), written by np.savez_compressed: zlib finds nothing '
        'to compress and writes stored blocks.  Kernel times are HIP event times of one warm pass; everything else is wall clock on the same '
        'box in the same run, one fresh process per `utils/loadz.load`.' % (T, args.videos, F, F, args.videos, T))
    say()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'random.npz')
        sequences = np.random.RandomState(SEED).randint(0, 256, size=(T, args.videos, 1, F, F), dtype=np.uint8)
        t0 = time.perf_counter()
        np.savez_compressed(path, sequences=sequences)
        say('The file: %.1f MB, written in %.2f s.' % (os.path.getsize(path) / 1e6, time.perf_counter() - t0))
        say()
        want = float(sequences.sum(dtype=np.int64))
        del sequences
        stored_table(path, dev, args.sample_mb)
        say('## `utils/loadz.load(keys=("sequences",))`, whole, alternating routes, a fresh process each')
        say()
        say('| VARSEP_NPZ_LOAD | VARSEP_NPZ_FOREIGN | VARSEP_NPZ_FINDER | seconds | peak HBM | `sequences` took | checksum right |')
        say('|---|---|---|---|---|---|---|')
        for _ in range(args.pairs):
            for route in STORED_ROUTES:
                r = run_child(path, route, '--child-stored')
                took = r['report']['sequences']
                load, foreign, finder = (route.split('+') + ['-', '-'])[:3]
                say('| %s | %s | %s | **%.2f s** | %.2f GB | %s (%s) | %s |' % (load, foreign, finder, r['seconds'], r['peak'] / 1e9, took[0], took[1],
                                                                          r['checksum'] == want))
        say()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    before = open(args.out).read().split(STORED_TITLE)[0] if os.path.exists(args.out) else ''
    with open(args.out, 'w') as f:
        f.write(before + '\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='the note to write (default: profiles/npz_load_timing.md, with --blocks profiles/npz_blocks_timing.md)')
    ap.add_argument('--blocks', action='store_true', help='the rule VARSEP_NPZ_FOREIGN on the np.savez_compressed file (see above)')
    ap.add_argument('--stored', action='store_true', help='with --blocks: the rule VARSEP_NPZ_FINDER on a file of random bytes (see above)')
    ap.add_argument('--sample-mb', type=float, default=4.0, help='--blocks: compressed MB a block walker reads on the host to count the misses')
    ap.add_argument('--videos', type=int, default=N_IMAGES // ND, help='videos of the set (the reference: 5 000)')
    ap.add_argument('--pairs', type=int, default=2, help='(device, host) pairs of fresh processes per file')
    ap.add_argument('--child', nargs=2, metavar=('DIR', 'ROUTE'), help=argparse.SUPPRESS)
    ap.add_argument('--child-stored', nargs=2, metavar=('FILE', 'ROUTE'), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    if args.child_stored:
        return child_stored(*args.child_stored)
    if args.stored and not args.blocks:
        ap.error('--stored is a form of --blocks')
    args.out = args.out or os.path.join(ROOT, 'profiles', 'npz_blocks_timing.md' if args.blocks else 'npz_load_timing.md')
    if args.stored:
        return main_stored(args)
    if args.blocks:
        return main_blocks(args)
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

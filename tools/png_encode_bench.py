"""Time and size of encoding the prepared 3D Chairs views (64 x 64 8-bit RGB) as PNG files on one MI355X against the host encoders:

  * per batch of 62, 496 and 1984 views, per kind of content and per matcher: one warm vs_png_filter, vs_deflate_streams and
    vs_png_assemble launch and ops.png_encode_u8 as a whole, each between two events, median of 10 (min - max);
  * the host baselines on the same box, 16 threads: PIL's `save` (when PIL imports) and data/chairs.py's `write_png_rgb8`, the same
    images once into files and once into `io.BytesIO` -- the difference is what creating the files costs, which no encoder removes;
  * the bytes of the device-written views over PIL's and over `write_png_rgb8`'s (zlib level 6);
  * `gen_chairs.generate` over a tree of 8 objects x 62 raw renders with encode=host and encode=device, alternating, every run in a
    fresh process (this file with --generate_once), split into its stages.

The views are the smooth and the noisy renders of tools/png_decode_bench.py, cropped and resized on the device as `generate` does; a
pool of POOL distinct views per kind is repeated to fill a batch.  Every device-written pool file is read back before anything is timed.

Prints a report (Markdown) on stdout:  python tools/png_encode_bench.py [--batches 62 496 1984] [--runs 3]"""
import argparse
import io
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
import png_inputs as P  # noqa: E402
import resample_inputs as I  # noqa: E402
from png_decode_bench import EDGE, POOL, THREADS, noisy_view  # noqa: E402
from resample_bench import cpu_model, median_ms  # noqa: E402
from spatiotemporal_variable_separation_amd import ops  # noqa: E402
from spatiotemporal_variable_separation_amd.data import chairs as C  # noqa: E402
from spatiotemporal_variable_separation_amd.preprocessing.chairs import gen_chairs  # noqa: E402

SIZE = 64
MATCHERS = ('runs', 'window')


def raw_pools():
    """{kind: uint8 [POOL, 600, 600, 3]}: the raw renders of tools/png_decode_bench.py."""
    return {'smooth': I.raw_views(0, POOL, size=EDGE), 'noisy': np.stack([noisy_view(v) for v in range(POOL)])}


def views(dev, raw):
    """uint8 [POOL, 64, 64, 3] on the device: the raw renders cropped and resized as `generate` does."""
    return ops.resample_lanczos_u8(torch.from_numpy(raw).to(dev), C.RAW_BOX, SIZE)


def builtin_bytes(img):
    """The bytes `write_png_rgb8` writes, without the file: its rows (filter type 2) and zlib level 6."""
    h, w, _ = img.shape
    rows = img.reshape(h, w * 3)
    raw = np.empty((h, w * 3 + 1), dtype=np.uint8)
    raw[:, 0] = 2
    raw[0, 1:] = rows[0]
    raw[1:, 1:] = rows[1:] - rows[:-1]
    return P.MAGIC + P.chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) + P.chunk(b'IDAT', zlib.compress(raw.tobytes(), 6)) \
        + P.chunk(b'IEND', b'')


def check_pool(dev, pool):
    with tempfile.TemporaryDirectory() as d:
        for match in MATCHERS:
            files, sizes = ops.png_encode_u8(pool, match=match)
            files, sizes = files.cpu().numpy(), sizes.cpu().numpy()
            for i in range(len(sizes)):
                path = os.path.join(d, 'v.png')
                with open(path, 'wb') as f:
                    f.write(files[i, :sizes[i]].tobytes())
                assert np.array_equal(C.read_png_rgb8(path), pool[i].cpu().numpy()), 'a device-written file does not read back'
        path = os.path.join(d, 'b.png')
        C.write_png_rgb8(path, pool[0].cpu().numpy())
        assert open(path, 'rb').read() == builtin_bytes(pool[0].cpu().numpy())


def fmt(t):
    return '%.3f ms (%.3f - %.3f)' % t


def device_times(dev, kind, pool, batches):
    print('### %s views on the device\n' % kind)
    print('| views | matcher | filter | deflate_streams | assemble | sum of the three | `png_encode_u8` | per view | bytes written |')
    print('|---|---|---|---|---|---|---|---|---|')
    S = SIZE * (1 + 3 * SIZE)
    for n in batches:
        batch = pool[torch.arange(n, device=dev) % len(pool)].contiguous()
        for match in MATCHERS:
            flt = median_ms(lambda: ops.png_filter(batch))
            raw = ops.png_filter(batch)
            dfl = median_ms(lambda: ops.deflate_streams(raw, S, None, match))
            slots, chunk_sizes = ops.deflate_streams(raw, S, None, match)
            asm = median_ms(lambda: ops.png_assemble(raw, slots, chunk_sizes, SIZE, SIZE, 3))
            whole = median_ms(lambda: ops.png_encode_u8(batch, match=match))
            _, sizes = ops.png_encode_u8(batch, match=match)
            assert int(sizes.min()) > 0
            print('| %d | %s | %s | %s | %s | %.3f ms | %s | %.2f us | %.3f MB |'
                  % (n, match, fmt(flt), fmt(dfl), fmt(asm), flt[0] + dfl[0] + asm[0], fmt(whole), 1e3 * whole[0] / n, int(sizes.sum()) / 1e6))
    print()


def host_times(kind, images, n, reps=5):
    """images: uint8 [POOL, 64, 64, 3] on the host; n views on THREADS threads into files and into memory."""
    image_module = C._pil_image()
    batch = [images[i % len(images)] for i in range(n)]
    print('### %s views on the host: %d views, %d threads, median of %d (min - max)\n' % (kind, n, THREADS, reps))
    print('| encoder | into files | into `io.BytesIO` | files - memory: creating %d files | bytes |' % n)
    print('|---|---|---|---|---|')

    def timed(fn):
        ts = []
        with ThreadPoolExecutor(max_workers=THREADS) as pool:
            list(pool.map(fn, range(THREADS)))
            for _ in range(reps):
                t0 = time.perf_counter()
                list(pool.map(fn, range(n), chunksize=1))
                ts.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ts)), min(ts), max(ts)

    totals = {}
    with tempfile.TemporaryDirectory() as d:
        paths = [os.path.join(d, '%d.png' % i) for i in range(n)]

        def pil_mem(i):
            b = io.BytesIO()
            image_module.fromarray(batch[i]).save(b, format='PNG')
            return b.tell()

        rows = []
        if image_module is not None:
            rows.append(('PIL `save`', lambda i: image_module.fromarray(batch[i]).save(paths[i]), pil_mem))
        rows.append(('`write_png_rgb8`', lambda i: C.write_png_rgb8(paths[i], batch[i]), lambda i: len(builtin_bytes(batch[i]))))
        for name, to_file, to_mem in rows:
            a, b = timed(to_file), timed(to_mem)
            totals[name] = sum(os.path.getsize(p) for p in paths)
            print('| %s | %s | %s | %.1f ms | %.3f MB |' % (name, '%.1f ms (%.1f - %.1f)' % a, '%.1f ms (%.1f - %.1f)' % b, a[0] - b[0], totals[name] / 1e6))
        if image_module is None:
            print('| PIL `save` | does not import on this host | - | - | - |')
        files = [np.frombuffer(builtin_bytes(batch[i]), dtype=np.uint8) for i in range(n)]
        block = np.zeros((n, max(len(f) for f in files)), dtype=np.uint8)
        sizes = np.array([len(f) for f in files], dtype=np.int64)
        for i, f in enumerate(files):
            block[i, :len(f)] = f
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            C.write_files(paths, block, sizes)
            ts.append(1e3 * (time.perf_counter() - t0))
        print('| `write_files` (open + write of finished files: the device route\'s host part) | %.1f ms (%.1f - %.1f) | - | - | %.3f MB |'
              % (float(np.median(ts)), min(ts), max(ts), sizes.sum() / 1e6))
    print()
    return totals


def size_ratios(dev, kind, pool, n, totals):
    batch = pool[torch.arange(n, device=dev) % len(pool)].contiguous()
    print('### %s views: bytes of %d device-written files over the host encoders\'\n' % (kind, n))
    print('| matcher | device bytes | / PIL | / `write_png_rgb8` |')
    print('|---|---|---|---|')
    for match in MATCHERS:
        _, sizes = ops.png_encode_u8(batch, match=match)
        total = int(sizes.sum())
        pil = totals.get('PIL `save`')
        print('| %s | %.3f MB | %s | %.3f |' % (match, total / 1e6, '%.3f' % (total / pil) if pil else '-', total / totals['`write_png_rgb8`']))
    print()


def write_tree(tree_dir, raw):
    n_objects, n_views = 8, 62
    root = os.path.join(tree_dir, 'rendered_chairs')
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, 'all_chair_names.mat'), 'wb') as f:
        f.write(b'placeholder\n')
    blobs = [builtin_bytes(np.ascontiguousarray(img)) for img in raw]
    for k in range(n_objects):
        d = os.path.join(root, 'chair_%02d' % k, 'renders')
        os.makedirs(d, exist_ok=True)
        for v in range(n_views):
            with open(os.path.join(d, 'image_%03d.png' % v), 'wb') as f:
                f.write(blobs[(k * n_views + v) % len(blobs)])


def generate_once(tree_dir, encode):
    """One fresh process: a warm-up run (code objects, the allocator), then the timed one.  Prints the stages as JSON."""
    dev = torch.device('cuda', 0)
    gen_chairs.generate(tree_dir, SIZE, dev, decode='device', encode=encode)
    timings = {}
    t0 = time.perf_counter()
    n = gen_chairs.generate(tree_dir, SIZE, dev, timings=timings, decode='device', encode=encode)
    timings['total'] = time.perf_counter() - t0
    timings['images'] = n
    print('TIMINGS ' + json.dumps(timings))


def generate_times(kind, tree_dir, runs):
    print('### `generate`, %s tree: 8 objects x 62 views, device decoder, %d alternating fresh processes per encoder; median (min - max)\n' % (kind, runs))
    got = {'host': [], 'device': []}
    for _ in range(runs):
        for encode in ('host', 'device'):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--generate_once', tree_dir, encode], capture_output=True, text=True,
                               timeout=900)
            assert r.returncode == 0, r.stderr[-3000:]
            got[encode].append(json.loads(r.stdout.split('TIMINGS ', 1)[1]))
    keys = ['decode', 'upload', 'kernel', 'encode', 'download', 'write', 'total']
    print('| stage | encode=host (%s) | encode=device |' % ('PIL' if C._pil_image() is not None else '`write_png_rgb8`'))
    print('|---|---|---|')
    for key in keys:
        cells = []
        for encode in ('host', 'device'):
            ts = [1e3 * t[key] for t in got[encode] if key in t]
            cells.append('%.1f ms (%.1f - %.1f)' % (float(np.median(ts)), min(ts), max(ts)) if ts else '-')
        print('| %s | %s | %s |' % (key, cells[0], cells[1]))
    print()


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batches', type=int, nargs='+', default=[62, 496, 1984])
    p.add_argument('--runs', type=int, default=3)
    p.add_argument('--generate_once', nargs=2, metavar=('TREE', 'ENCODE'))
    args = p.parse_args()
    if args.generate_once:
        generate_once(*args.generate_once)
        return
    dev = torch.device('cuda', 0)
    print('# PNG encoding on the device (`tools/png_encode_bench.py`)\n')
    print('Host CPU: %s; PIL %s.  Device figures: events round warm launches, median of 10 (min - max).\n'
          % (cpu_model(), 'imports' if C._pil_image() is not None else 'does not import'))
    raw = raw_pools()
    pools = {kind: views(dev, r) for kind, r in raw.items()}
    for pool in pools.values():
        check_pool(dev, pool)
    print('## Device: the three launches and `ops.png_encode_u8`\n')
    for kind, pool in pools.items():
        device_times(dev, kind, pool, args.batches)
    print('## Host baselines on the same box, and the sizes\n')
    for kind, pool in pools.items():
        totals = host_times(kind, pool.cpu().numpy(), 496)
        size_ratios(dev, kind, pool, 496, totals)
    print('## `gen_chairs.generate` under both encoders (the device is synchronised after every stage)\n')
    for kind, r in raw.items():
        with tempfile.TemporaryDirectory() as d:
            write_tree(d, r)
            generate_times(kind, d, args.runs)


if __name__ == '__main__':
    main()

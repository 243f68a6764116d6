"""Time of decoding the raw 3D Chairs renders (600 x 600 8-bit RGB PNG files) on one MI355X against the host decoders:

  * per batch of 62, 496 and 1984 files and per kind of content: packing on the host, the upload of the COMPRESSED bytes, one warm
    vs_inflate_zlib launch and one warm vs_png_unfilter launch, each between two events, median of 10;
  * the host baselines on the same box, at most 16 threads: PIL's decode when PIL imports, and the built-in reader `read_png_rgb8`
    (on 16 files only where its pure-Python rows make more too slow; the line says so);
  * `gen_chairs.generate` over a tree of 8 objects x 62 views under both decoders, split into its stages.

Two kinds of content, a pool of POOL distinct files each, repeated to fill a batch: `smooth`, the synthetic renders of
tools/resample_bench.py (gradients and one hard-edged square, one filter type per file), and `noisy`, a textured object on a gradient
written with the filter type chosen per row (least sum of absolute residuals), so that Average and Paeth rows and dense dynamic blocks
occur.  Every decoded pool image is compared with the built-in reader's before anything is timed.

Prints a report (Markdown) on stdout:  python tools/png_decode_bench.py [--batches 62 496 1984] [--cpu_only]
--cpu_only times only the built-in reader on one 600 x 600 all-Paeth file (no GPU needed)."""
import argparse
import io
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import png_inputs as P  # noqa: E402
import resample_inputs as I  # noqa: E402
from resample_bench import cpu_model, median_ms  # noqa: E402
from spatiotemporal_variable_separation_amd import ops  # noqa: E402
from spatiotemporal_variable_separation_amd.data import chairs as C  # noqa: E402
from spatiotemporal_variable_separation_amd.preprocessing.chairs import gen_chairs  # noqa: E402

EDGE, POOL, THREADS = 600, 16, 16


def noisy_view(v):
    """uint8 [600, 600, 3]: a gradient background, and an object (a disc that moves with the view) with a random texture on it."""
    rng = np.random.RandomState(P.SEED + v)
    yy, xx = np.mgrid[0:EDGE, 0:EDGE]
    img = np.stack([(xx // 3 + yy // 5 + 40 * k + v) % 256 for k in range(3)], axis=-1).astype(np.int32)
    img += rng.randint(-2, 3, size=img.shape)                              # sensor-like noise everywhere
    cy, cx = 300 + 60 * np.sin(v), 300 + 60 * np.cos(v)
    disc = (yy - cy) ** 2 + (xx - cx) ** 2 < 170 ** 2
    texture = np.kron(rng.randint(0, 256, size=(EDGE // 4, EDGE // 4, 3)), np.ones((4, 4, 1), dtype=np.int64)) // 2 + rng.randint(0, 128, size=img.shape)
    img[disc] = texture[disc]
    return img.clip(0, 255).astype(np.uint8)


def pools():
    smooth_img = I.raw_views(0, POOL, size=EDGE)
    smooth = [P.png_bytes(smooth_img[v], ftypes=1 + v % 2) for v in range(POOL)]
    noisy_img = [noisy_view(v) for v in range(POOL)]
    noisy = [P.png_bytes(im, ftypes='adaptive') for im in noisy_img]
    rows = np.bincount(np.concatenate([P.adaptive_ftypes(im) for im in noisy_img[:4]]), minlength=5)
    return {'smooth': (smooth, list(smooth_img)), 'noisy': (noisy, noisy_img)}, rows


def paeth_cpu_figure():
    img = noisy_view(0)
    blob = P.png_bytes(img, ftypes=4)
    with tempfile.NamedTemporaryFile(suffix='.png') as f:
        f.write(blob)
        f.flush()
        t0 = time.perf_counter()
        out = C.read_png_rgb8(f.name)
        dt = time.perf_counter() - t0
    assert np.array_equal(out, img)
    print('`read_png_rgb8` on ONE 600 x 600 file whose rows are all Paeth (%d bytes), one thread of this host (%s): %.2f s.\n'
          % (len(blob), cpu_model(), dt))


def device_times(dev, kind, blobs, images, batches):
    print('### %s: %d distinct files, mean %.1f KB compressed (%.0f x smaller than the pixels)\n'
          % (kind, len(blobs), np.mean([len(b) for b in blobs]) / 1e3, EDGE * EDGE * 3 / np.mean([len(b) for b in blobs])))
    pixels, status = ops.png_decode_rgb8(blobs, device=dev, check_status=True)
    assert all(np.array_equal(pixels[i].cpu().numpy(), images[i]) for i in range(len(blobs))), 'the device decoder disagrees with the source images'
    del pixels
    print('| files | compressed | pack (host) | upload | inflate | unfilter | device total | per file |')
    print('|---|---|---|---|---|---|---|---|')
    for n in batches:
        batch = [blobs[i % len(blobs)] for i in range(n)]
        t0 = time.perf_counter()
        W, H, packed, offsets = ops.png_pack(batch)
        t_pack = time.perf_counter() - t0
        host_bytes = torch.from_numpy(packed)
        up = median_ms(lambda: (host_bytes.to(dev), torch.from_numpy(offsets).to(dev)))
        packed_d, offsets_d = host_bytes.to(dev), torch.from_numpy(offsets).to(dev)
        size = H * (1 + 3 * W)
        out_len = torch.full((n,), size, dtype=torch.int64, device=dev)
        inf = median_ms(lambda: ops.inflate_zlib(packed_d, offsets_d, out_len, size))
        raw, st, _ = ops.inflate_zlib(packed_d, offsets_d, out_len, size)
        unf = median_ms(lambda: ops.png_unfilter(raw, st, H, W, 3))
        assert not st.any().item()
        total = up[0] + inf[0] + unf[0]
        print('| %d | %.1f MB | %.1f ms | %.3f ms (%.3f - %.3f) | %.2f ms (%.2f - %.2f) | %.2f ms (%.2f - %.2f) | %.2f ms | %.1f us |'
              % ((n, packed.size / 1e6, 1e3 * t_pack) + up + inf + unf + (total, 1e3 * total / n)))
        del raw, packed_d
    print()


def host_times(kind, blobs, batches):
    image_module = C._pil_image()
    print('### %s: host decoders, at most %d threads\n' % (kind, THREADS))
    print('| decoder | files | time | per file |')
    print('|---|---|---|---|')
    if image_module is not None:
        def pil(b):
            with image_module.open(io.BytesIO(b)) as im:
                return np.array(im)
        for n in batches:
            batch = [blobs[i % len(blobs)] for i in range(n)]
            with ThreadPoolExecutor(max_workers=THREADS) as pool:
                list(pool.map(pil, batch[:THREADS]))
                t0 = time.perf_counter()
                list(pool.map(pil, batch, chunksize=1))
                dt = time.perf_counter() - t0
            print('| PIL | %d | %.1f ms | %.2f ms |' % (n, 1e3 * dt, 1e3 * dt / n))
    else:
        print('| PIL | - | does not import on this host | - |')
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i in range(THREADS):
            paths.append(os.path.join(d, '%d.png' % i))
            with open(paths[-1], 'wb') as f:
                f.write(blobs[i % len(blobs)])
        with ThreadPoolExecutor(max_workers=THREADS) as pool:
            t0 = time.perf_counter()
            list(pool.map(C.read_png_rgb8, paths, chunksize=1))
            dt = time.perf_counter() - t0
    print('| `read_png_rgb8` (the built-in reader: the decode stage where PIL is missing) | %d, one per thread | %.1f ms | %.2f ms |'
          % (THREADS, 1e3 * dt, 1e3 * dt / THREADS))
    print()


def generate_times(dev, kind, blobs, tree_dir):
    n_objects, n_views = 8, 62
    root = os.path.join(tree_dir, 'rendered_chairs')
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, 'all_chair_names.mat'), 'wb') as f:
        f.write(b'placeholder\n')
    for k in range(n_objects):
        d = os.path.join(root, 'chair_%02d' % k, 'renders')
        os.makedirs(d, exist_ok=True)
        for v in range(n_views):
            with open(os.path.join(d, 'image_%03d.png' % v), 'wb') as f:
                f.write(blobs[(k * n_views + v) % len(blobs)])
    print('### `generate`, %s tree: %d objects x %d views, second run of each decoder\n' % (kind, n_objects, n_views))
    print('| stage | host decoder (%s) | device decoder |' % ('PIL' if C._pil_image() is not None else 'built-in reader'))
    print('|---|---|---|')
    cols = {}
    for decode in ('host', 'device'):
        gen_chairs.generate(tree_dir, 64, dev, decode=decode)
        timings = {}
        t0 = time.perf_counter()
        n = gen_chairs.generate(tree_dir, 64, dev, timings=timings, decode=decode)
        timings['total (%d images)' % n] = time.perf_counter() - t0
        cols[decode] = timings
    for key in cols['host']:
        print('| %s | %.1f ms | %.1f ms |' % (key, 1e3 * cols['host'][key], 1e3 * cols['device'][key]))
    print()


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batches', type=int, nargs='+', default=[62, 496, 1984])
    p.add_argument('--cpu_only', action='store_true')
    args = p.parse_args()
    print('# PNG decoding on the device (`tools/png_decode_bench.py`)\n')
    if args.cpu_only:
        paeth_cpu_figure()
        return
    dev = torch.device('cuda', 0)
    print('Host CPU: %s; PIL %s.  Events round warm launches, median of 10 (min - max).\n' % (cpu_model(), 'imports' if C._pil_image() is not None else 'does not import'))
    content, rows = pools()
    print('Filter types of the rows of the noisy files (first 4): None %d, Sub %d, Up %d, Average %d, Paeth %d.\n' % tuple(rows))
    print('## Device: the compressed batch, from packed bytes on the host\n')
    for kind, (blobs, images) in content.items():
        device_times(dev, kind, blobs, images, args.batches)
    print('## Host baselines on the same box\n')
    for kind, (blobs, _) in content.items():
        host_times(kind, blobs, [b for b in args.batches if b <= 496])
    print('## `gen_chairs.generate` under both decoders (the device is synchronised after every stage)\n')
    for kind, (blobs, _) in content.items():
        with tempfile.TemporaryDirectory() as d:
            generate_times(dev, kind, blobs, d)


if __name__ == '__main__':
    main()

"""Time of the 3D Chairs preparation (crop (100, 100, 500, 500) + Lanczos resize of 600 x 600 x 3 renders to 64 x 64) on one MI355X:

  * one warm vs_resample_u8 launch between two events for 62, 496 and 1984 synthetic images (1, 8 and 32 objects), median of 10, and the
    rate at which it reads the box (n x 400 x 400 x 3 bytes);
  * PIL's `crop().resize(LANCZOS)` of 62 of the same images on this host, on 1 thread and on 16 threads, when PIL imports; otherwise the
    NumPy restatement (tests/resample_ref.py) on 1 thread, and a line that says so;
  * one `gen_chairs.generate` run over a synthetic tree of 8 objects x 62 views, split into decode, upload, kernel, download and write.

Prints a report (Markdown) on stdout:  python tools/resample_bench.py [--tree_dir DIR]"""
import argparse
import os
import platform
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import chairs_inputs  # noqa: E402
import resample_inputs as I  # noqa: E402
import resample_ref as R  # noqa: E402
from spatiotemporal_variable_separation_amd import ops  # noqa: E402
from spatiotemporal_variable_separation_amd.data import chairs as C  # noqa: E402
from spatiotemporal_variable_separation_amd.preprocessing.chairs import gen_chairs  # noqa: E402

BOX, SIZE, EDGE = C.RAW_BOX, 64, 600


def cpu_model():
    try:
        with open('/proc/cpuinfo') as f:
            for line in f:
                if line.startswith('model name'):
                    return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or 'unknown'


def median_ms(fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), min(ts), max(ts)


def kernel_times(dev):
    print('## Kernel: one warm launch between two events, median of 10 (min - max)\n')
    print('| images | time | per image | box bytes read | read rate |')
    print('|---|---|---|---|---|')
    gen = torch.Generator(device=dev).manual_seed(1)
    for n in (62, 496, 1984):
        x = torch.randint(0, 256, (n, EDGE, EDGE, 3), dtype=torch.uint8, device=dev, generator=gen)
        med, lo, hi = median_ms(lambda: ops.resample_lanczos_u8(x, BOX, SIZE))
        nbytes = n * (BOX[2] - BOX[0]) * (BOX[3] - BOX[1]) * 3
        print('| %d | %.3f ms (%.3f - %.3f) | %.2f us | %.1f MB | %.2f TB/s |' % (n, med, lo, hi, 1e3 * med / n, nbytes / 1e6, nbytes / med / 1e9))
        if n == 62:
            host = x.cpu().numpy()
            out = ops.resample_lanczos_u8(x, BOX, SIZE).cpu().numpy()
        del x
    print()
    return host, out


def host_times(host, out):
    image_module = C._pil_image()
    print('## Host: the same 62 images, crop + resize only (no decoding)\n')
    if image_module is None:
        print('PIL does not import on this host; the NumPy restatement (tests/resample_ref.py) is timed instead, on 1 thread.\n')
        t0 = time.perf_counter()
        ref = R.resample(host, BOX, SIZE)
        dt = time.perf_counter() - t0
        print('* NumPy restatement: %.1f ms for 62 images, %.2f ms per image; equal to the kernel: %s' % (1e3 * dt, 1e3 * dt / 62, np.array_equal(ref, out)))
        print()
        return
    import PIL
    lanczos = getattr(image_module, 'Resampling', image_module).LANCZOS
    images = [image_module.fromarray(a) for a in host]

    def one(im):
        return np.array(im.crop(BOX).resize((SIZE, SIZE), lanczos))

    one(images[0])
    t0 = time.perf_counter()
    ref = np.stack([one(im) for im in images])
    t1 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=16) as pool:
        list(pool.map(one, images))
    t2 = time.perf_counter()
    print('PIL %s imports on this host.\n' % PIL.__version__)
    print('* PIL, 1 thread: %.1f ms for 62 images, %.2f ms per image; equal to the kernel: %s' % (1e3 * (t1 - t0), 1e3 * (t1 - t0) / 62, np.array_equal(ref, out)))
    print('* PIL, 16 threads: %.1f ms for 62 images, %.2f ms per image' % (1e3 * (t2 - t1), 1e3 * (t2 - t1) / 62))
    print()


def generate_times(dev, tree_dir):
    n_objects, n_views = 8, 62
    t0 = time.perf_counter()
    root = os.path.join(tree_dir, 'rendered_chairs')
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, 'all_chair_names.mat'), 'wb') as f:
        f.write(b'placeholder\n')
    image_module = C._pil_image()
    for k in range(n_objects):
        d = os.path.join(root, 'chair_%02d' % k, 'renders')
        os.makedirs(d, exist_ok=True)
        views = I.raw_views(k, n_views, size=EDGE)
        for v in range(n_views):
            path = os.path.join(d, 'image_%03d.png' % v)
            if image_module is not None:
                image_module.fromarray(views[v]).save(path)
            else:
                chairs_inputs.write_png(path, views[v], ftype=1)
    t_tree = time.perf_counter() - t0
    size = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(root) for f in fs)
    gen_chairs.generate(tree_dir, SIZE, dev)             # warm: the library, the tables, the page cache
    timings = {}
    t0 = time.perf_counter()
    n = gen_chairs.generate(tree_dir, SIZE, dev, timings=timings)
    total = time.perf_counter() - t0
    print('## `generate` over a synthetic tree: %d objects x %d views of %d x %d (second run; %.1f MB of PNG files, written in %.1f s)\n'
          % (n_objects, n_views, EDGE, EDGE, size / 1e6, t_tree))
    print('Decoder and writer: %s; at most %d threads.\n' % ('PIL' if image_module is not None else 'the built-in zlib + NumPy reader and writer', C.MAX_DECODE_WORKERS))
    print('| stage | time | share |')
    print('|---|---|---|')
    for key in ('decode', 'upload', 'kernel', 'download', 'write'):
        print('| %s | %.1f ms | %.1f %% |' % (key, 1e3 * timings[key], 100 * timings[key] / total))
    print('| total (%d images) | %.1f ms | %.2f ms per image |' % (n, 1e3 * total, 1e3 * total / n))
    print()


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--tree_dir', default=None, help='Where the synthetic tree is written (default: a temporary directory).')
    args = p.parse_args()
    dev = torch.device('cuda', 0)
    print('# vs_resample_u8 and the 3D Chairs preparation (one MI355X, `tools/resample_bench.py`)\n')
    print('Host CPU: %s; PIL %s.\n' % (cpu_model(), 'imports' if C._pil_image() is not None else 'does not import'))
    host, out = kernel_times(dev)
    host_times(host, out)
    if args.tree_dir:
        generate_times(dev, args.tree_dir)
    else:
        with tempfile.TemporaryDirectory() as d:
            generate_times(dev, d)


if __name__ == '__main__':
    main()

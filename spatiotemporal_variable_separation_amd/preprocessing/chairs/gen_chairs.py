"""3D Warehouse Chairs preprocessing on the device (reference: preprocessing/chairs/gen_chairs.py, same flags plus --device):

    python -m spatiotemporal_variable_separation_amd.preprocessing.chairs.gen_chairs --data_dir D --device 0

For every object of D/rendered_chairs, the i-th of its sorted raw renders (600 x 600 in the original set) is cropped to (100, 100, 500, 500),
resized to image_size x image_size with PIL's Lanczos filter and written as renders/{i}.png: the files `Chairs(D, ...)`, the reference's
loader and test/chairs/test_disentanglement.py read.  The reference does this with PIL, one image after the other on the host; here the
crop and the resize of a batch of whole objects are ONE launch (ops.resample_lanczos_u8, csrc/vs_resample.hip), which reproduces PIL's
8-bit arithmetic bit for bit.  The PNG files are decoded on the host (PIL when it imports, data/chairs.py's own reader otherwise) or on the
device (ops.png_decode_rgb8: only the compressed bytes are uploaded; two more launches, the same bytes).  The environment variable
VARSEP_CHAIRS_DECODE=host|device selects the decoder; unset, the device decodes where PIL does not import.  The resized views are
encoded on the host (PIL's `save` or data/chairs.py's writer, one by one on a thread pool) or, with VARSEP_CHAIRS_ENCODE=device, on the
device (ops.png_encode_u8: row filters, one zlib stream per view, framing; only the finished files are downloaded); unset means host.
One deviation from the reference: names of the form <digits>.png are left out of an object's listing, so a second
run reproduces the first (the reference would feed its own outputs back in).  There is no CPU mode: --device is required.
`--chairs_raw` of main.py and test/chairs/test_disentanglement_raw.py build the same set straight in HBM, without files (`Chairs.from_raw`).
"""
import argparse
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ... import ops
from ...data import chairs as C


def _save_all(paths, images, image_module):
    """images uint8 [n, s, s, 3] (host) -> one PNG per path: PIL's `save` when PIL imports, data/chairs.py's writer otherwise."""
    def save(i):
        if image_module is not None:
            image_module.fromarray(images[i]).save(paths[i])
        else:
            C.write_png_rgb8(paths[i], images[i])

    with ThreadPoolExecutor(max_workers=min(C.MAX_DECODE_WORKERS, len(paths))) as pool:
        for _ in pool.map(save, range(len(paths)), chunksize=1):
            pass


def generate(data_dir, image_size, device, box=C.RAW_BOX, timings=None, decode=None, encode=None):
    """The reference's `generate` (gen_chairs.py:23-33) plus the device and the crop box.  Works in batches of whole objects: decode, one
    upload, one launch, one download, write.  Returns the number of files written.  timings: optional dict that receives the seconds
    spent in 'decode', 'upload', 'kernel', 'download' and 'write' (the device is then synchronised after every stage).  decode: 'host',
    'device' or None (the environment variable VARSEP_CHAIRS_DECODE, then the default rule of data/chairs.py's `chairs_decoder`).
    encode: 'host' (PIL or data/chairs.py's writer, on the thread pool), 'device' or None (the environment variable VARSEP_CHAIRS_ENCODE,
    then 'host').  With 'device' the resized batch stays in HBM, ops.png_encode_u8 makes the files there (three launches), the files and
    their sizes come down in one copy each and the thread pool only opens and writes; timings then also receives 'encode'."""
    device = C.require_gpu('Chairs preprocessing', device)
    box = tuple(int(v) for v in box)
    root, objects = C.list_objects(data_dir)
    on_device = C.chairs_encoder(encode) == 'device'
    image_module = C._pil_image()                        # (the host decoder's; the device encoder needs none)
    written = 0
    for start in range(0, len(objects), C.OBJECTS_PER_BATCH):
        sources, targets = [], []
        for obj in objects[start:start + C.OBJECTS_PER_BATCH]:
            renders = os.path.join(root, obj, 'renders')
            names = C.raw_render_names(renders)
            sources += [os.path.join(renders, f) for f in names]
            targets += [os.path.join(renders, '%d.png' % i) for i in range(len(names))]
        if not sources:
            continue
        out = C.prepare_renders(sources, box, image_size, device, image_module, timings, decode)
        t0 = time.perf_counter()
        if on_device:
            files, sizes = ops.png_encode_u8(out)
            if timings is not None:
                torch.cuda.synchronize(device)
                timings['encode'] = timings.get('encode', 0.0) + time.perf_counter() - t0
                t0 = time.perf_counter()
            files, sizes = files.cpu().numpy(), sizes.cpu().numpy()
            if sizes.min() < 0:
                raise RuntimeError('%s: the device encoder left no file' % targets[int(sizes.argmin())])
            t1 = time.perf_counter()
            C.write_files(targets, files, sizes)
        else:
            host = out.cpu().numpy()
            t1 = time.perf_counter()
            _save_all(targets, host, image_module)
        if timings is not None:
            timings['download'] = timings.get('download', 0.0) + t1 - t0
            timings['write'] = timings.get('write', 0.0) + time.perf_counter() - t1
        written += len(targets)
    return written


def build_parser():
    p = argparse.ArgumentParser(prog='3D Warehouse chairs preprocessing.', formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                description='Crops and resizes the original renders on an MI355X and saves them as renders/{i}.png.')
    p.add_argument('--data_dir', type=str, metavar='DIR', required=True, help='Folder where videos from the original dataset are stored.')
    p.add_argument('--image_size', type=int, metavar='SIZE', default=64, help='Width and height of resulting processed videos.')
    p.add_argument('--device', type=int, metavar='DEVICE', default=None, help='GPU the resize runs on (required: there is no CPU mode).')
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.device is None:
        parser.error('the resize runs on an MI355X: pass --device N (there is no CPU mode)')
    if args.image_size < 1:
        parser.error('--image_size must be positive')
    n = generate(args.data_dir, args.image_size, torch.device('cuda', args.device))
    print('wrote %d images of %d x %d below %s' % (n, args.image_size, args.image_size, os.path.join(args.data_dir, 'rendered_chairs')))


if __name__ == '__main__':
    main()

"""Writes tests/golden/resample/<case>.npz: PIL's `crop(box).resize(size, LANCZOS)` of the seeded case inputs (tests/resample_inputs.py).
Needs PIL; run from the repository root on a machine that has it:  python tests/make_golden_resample.py
The files hold the outputs only (key `out`, uint8 [n, h, w, C]) and the PIL version that made them; the inputs are rebuilt from seeds."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_inputs as I  # noqa: E402


def pil_resample(images, box, size):
    import PIL
    from PIL import Image
    size = (size, size) if isinstance(size, int) else size
    lanczos = getattr(Image, 'Resampling', Image).LANCZOS
    out = []
    for img in images:
        # modes L, RGB and, for four channels, CMYK: four plain 8-bit channels (RGBA would be premultiplied by its alpha around the resize)
        H, W, C = img.shape
        im = Image.frombytes({1: 'L', 3: 'RGB', 4: 'CMYK'}[C], (W, H), img.tobytes())
        arr = np.array(im.crop(box).resize(size, lanczos))
        out.append(arr[..., None] if img.shape[-1] == 1 else arr)
    return np.stack(out), PIL.__version__


def main():
    os.makedirs(I.GOLDEN, exist_ok=True)
    for name, (_, box, size) in I.CASES.items():
        out, version = pil_resample(I.case_input(name), box, size)
        np.savez_compressed(os.path.join(I.GOLDEN, '%s.npz' % name), out=out, pil_version=np.array(version))
        print(name, out.shape, os.path.getsize(os.path.join(I.GOLDEN, '%s.npz' % name)), 'bytes')


if __name__ == '__main__':
    main()

"""Pixel choice of the WaveEq-100 set (reference: preprocessing/wave/gen_pixels.py, same flags):

    python -m spatiotemporal_variable_separation_amd.preprocessing.wave.gen_pixels --data_dir D

Writes D/pixels/pixels.npz with the fields `rand_w` and `rand_h` that `WaveEqPartial` reads.  Host only: two draws from NumPy's seeded
legacy generator, the reference's draws in the reference's order.
"""
import argparse
import os

import numpy as np


def draw_pixels(number=100, frame_size=64, seed=42):
    """(rand_w, rand_h): `number` coordinates each below `frame_size`, rand_w drawn first (gen_pixels.py:40, 48-49)."""
    rng = np.random.RandomState(seed)                    # the stream np.random.seed(seed) starts, without touching the global one
    rand_w = rng.randint(frame_size, size=number)
    rand_h = rng.randint(frame_size, size=number)
    return rand_w, rand_h


def generate(data_dir, number=100, frame_size=64, seed=42):
    out_dir = os.path.join(data_dir, 'pixels')
    os.makedirs(out_dir, exist_ok=True)
    rand_w, rand_h = draw_pixels(number, frame_size, seed)
    path = os.path.join(out_dir, 'pixels.npz')
    np.savez_compressed(path, rand_w=rand_w, rand_h=rand_h)
    return path


def build_parser():
    p = argparse.ArgumentParser(prog='WaveEq-100 pixel choice',
                                description='Draws the pixel coordinates of the WaveEqPartial set (WaveEq-100 for 100 pixels) and saves them as '
                                            '`rand_w` and `rand_h` in pixels/pixels.npz under the data directory.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--data_dir', type=str, metavar='DIR', required=True, help='Data directory; pixels/pixels.npz is written below it.')
    p.add_argument('--number', type=int, metavar='NUM', default=100, help='How many pixels to draw.')
    p.add_argument('--frame_size', type=int, metavar='SIZE', default=64, help='Frame edge: coordinates are drawn below it.')
    p.add_argument('--seed', type=int, metavar='SEED', default=42, help='NumPy seed of the draw.')
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    print('wrote', generate(args.data_dir, args.number, args.frame_size, args.seed))


if __name__ == '__main__':
    main()

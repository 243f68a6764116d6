"""WaveEq simulations on the device (reference: preprocessing/wave/gen_wave.py, same flags plus --device):

    python -m spatiotemporal_variable_separation_amd.preprocessing.wave.gen_wave --data_dir D --device 0

Writes D/data/homogenous_wave{i}.pt, each a dict {'simul': CPU fp32 [seq_len, 64, 64], 'c': velocity}: the reference's files, which
`WaveEq(D, ...)`, the reference's loader and test/wave/test.py read.  The reference integrates one sequence after the other with
torchdiffeq on the host; here every sequence of the set is one workgroup of ONE launch (ops.wave_simulate, csrc/vs_wave_sim.hip, which
states the equations and the Runge-Kutta tableau).  The parameters are the reference's to the last bit: f0 ~ U(1, 30) then c ~ U(300, 400)
per sequence from NumPy's legacy generator seeded once.  There is no CPU mode: --device is required.  `--data_dir simulated` of main.py
and test/wave/test.py builds the same set straight in HBM, without files (data/wave_eq.py: `WaveEq.simulated`).
"""
import argparse
import os

import numpy as np
import torch

FRAME_SIZE = 64


def wave_parameters(size, seed=42):
    """(f0 [size], c [size]) as float64: per sequence the source amplitude U(1, 30) and THEN the velocity U(300, 400), interleaved, from
    one stream seeded once (gen_wave.py:123, 130, 162) -- sequence i gets the reference's parameters."""
    rng = np.random.RandomState(seed)                    # the stream np.random.seed(seed) starts, without touching the global one
    f0, c = np.empty(size), np.empty(size)
    for i in range(size):
        f0[i] = rng.uniform(1, 30)
        c[i] = rng.uniform(300, 400)
    return f0, c


def check_frame_size(frame_size):
    if frame_size != FRAME_SIZE:
        raise ValueError('only 64x64 frames can be simulated (got --frame_size %d): the source disc of the reference is fixed to a 64x64 '
                         'grid, so its generator works at no other size either' % frame_size)


def simulate(size, seq_len, seed=42, dt=0.001, device=None, normalise=False):
    """-> (simul fp32 [size, seq_len, 64, 64] on the device, minmax fp32 [size, 2] on the device, c float64 [size]); one launch."""
    from ... import ops
    f0, c = wave_parameters(size, seed)
    simul, minmax = ops.wave_simulate(f0, c, seq_len, dt, normalise=normalise, device=device)
    return simul, minmax, c


def generate(size, frame_size, seq_len, dt, data_dir, seed=42, device=None):
    """The reference's `generate` (gen_wave.py:95-138) plus the seed (the reference seeds the global stream before the call) and the device."""
    check_frame_size(frame_size)
    simul, _, c = simulate(size, seq_len, seed, dt, device)
    out_dir = os.path.join(data_dir, 'data')
    os.makedirs(out_dir, exist_ok=True)
    simul = simul.cpu()
    for i in range(size):
        torch.save({'simul': simul[i].clone(), 'c': float(c[i])}, os.path.join(out_dir, 'homogenous_wave%d.pt' % i))
    return out_dir


def build_parser():
    p = argparse.ArgumentParser(prog='WaveEq preprocessing',
                                description='Simulates the WaveEq dataset on an MI355X and saves it as pt files in the folder `data` of the '
                                            'given directory.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--data_dir', type=str, metavar='DIR', required=True, help='Data directory; data/homogenous_wave{i}.pt are written below it.')
    p.add_argument('--seq_len', type=int, metavar='LEN', default=300, help='Frames per sequence.')
    p.add_argument('--seed', type=int, metavar='SEED', default=42, help='NumPy seed of the source amplitudes and velocities.')
    p.add_argument('--frame_size', type=int, metavar='SIZE', default=64, help='Frame edge; only 64 is supported.')
    p.add_argument('--size', type=int, metavar='SIZE', default=300, help='Number of sequences.')
    p.add_argument('--dt', type=float, metavar='DT', default=0.001,
                   help='Solver step and time between frames.  A float here: the reference declares type=int, which rejects every value '
                        'but its default.')
    p.add_argument('--device', type=int, metavar='DEVICE', default=None, help='GPU the simulation runs on (required: there is no CPU mode).')
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.device is None:
        parser.error('the simulation runs on an MI355X: pass --device N (there is no CPU mode)')
    try:
        check_frame_size(args.frame_size)
    except ValueError as e:
        parser.error(str(e))
    device = torch.device('cuda', args.device)
    print('wrote %d sequences of %d frames to %s' % (args.size, args.seq_len,
                                                     generate(args.size, args.frame_size, args.seq_len, args.dt, args.data_dir, args.seed, device)))


if __name__ == '__main__':
    main()

"""Time of the WaveEq simulation on the device at the paper's size (300 sequences of 300 frames of 64x64, the reference's seeded
parameters): one vs_wave_simulate launch between two events, warm, with and without the in-place normalisation, for 1, 256 and 300
sequences; the copy and fill rates of a buffer of the output's size (what the frame stores could cost); and the NumPy fp32 restatement
of the same set (tests/wave_sim_ref.py) on the host."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import wave_sim_ref as R  # noqa: E402
from spatiotemporal_variable_separation_amd import _lib, ops  # noqa: E402
from spatiotemporal_variable_separation_amd.preprocessing.wave.gen_wave import wave_parameters  # noqa: E402

N, T = 300, 300
f0, c = wave_parameters(N, 42)
lib = _lib.load_library()
dev = torch.device('cuda', 0)
source, h = ops.wave_source_table(f0, T, 0.001)
c2, source, h = (torch.from_numpy(a).to(dev) for a in ((c * c).astype(np.float32), source, h))
out = torch.empty((N, T, 64, 64), dtype=torch.float32, device=dev)
minmax = torch.empty((N, 2), dtype=torch.float32, device=dev)


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


def launch(n, normalise):
    _lib.check(lib.vs_wave_simulate(n, T, 64, c2.data_ptr(), source.data_ptr(), h.data_ptr(), None, out.data_ptr(), minmax.data_ptr(), normalise,
                                    _lib.stream_ptr()), 'vs_wave_simulate')


for n in (1, 256, N):
    for normalise in (0, 1):
        print('n_seq %3d normalise %d: median %.3f ms (min %.3f, max %.3f)' % ((n, normalise) + median_ms(lambda: launch(n, normalise))), flush=True)
other = torch.empty_like(out)
nbytes = out.numel() * 4
ms = median_ms(lambda: other.copy_(out))[0]
print('copy of %.3f GB: %.3f ms = %.2f TB/s written (%.2f TB/s read + written)' % (nbytes / 1e9, ms, nbytes / ms / 1e9, 2 * nbytes / ms / 1e9), flush=True)
ms = median_ms(lambda: other.zero_())[0]
print('fill of %.3f GB: %.3f ms = %.2f TB/s written' % (nbytes / 1e9, ms, nbytes / ms / 1e9), flush=True)
t0 = time.time()
for k in range(N):
    R.simulate(f0[k], c[k], T, dtype=np.float32)
print('NumPy fp32 restatement, %d x %d frames on the host: %.2f s' % (N, T, time.time() - t0), flush=True)

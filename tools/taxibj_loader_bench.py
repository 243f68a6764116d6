"""TaxiBJ input path on the device, two measurements:

1. `vs_gather_timeline` at the recipe's sizes (32x32x2 frames, 4 + 4 frames per item, batch 100) from a timeline of the paper's length
   (22 000 frames = 180 MB fp32 in HBM) through a random window table read backwards, fp32 and bf16 output: device events around 200
   launches.
2. Training epochs of `main --data taxibj` on the synthetic years of tests/taxibj_inputs.py (192 train windows: `DeviceBatchLoader` + one
   gather launch per batch) against the same epochs on `--data_dir synthetic` (192 items), same network and batch size: the frames/s `main`
   logs once per epoch, median over the epochs after the recording.

    python tools/taxibj_loader_bench.py [--skip_epochs]
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from spatiotemporal_variable_separation_amd import ops  # noqa: E402

n_frames, frame, B, seq_len, n_windows, reps = 22000, 2 * 32 * 32, 100, 8, 20000, 200
timeline = torch.rand(n_frames, frame, device='cuda')
g = torch.Generator().manual_seed(0)
first = torch.randint(seq_len - 1, n_frames, (n_windows,), generator=g, dtype=torch.int32).cuda()
for dt in (torch.float32, torch.bfloat16):
    idx = [torch.randint(0, n_windows, (B,), generator=g, dtype=torch.int32).cuda() for _ in range(reps)]
    for i in idx[:5]:
        ops.gather_timeline(timeline, first, i, seq_len, -1, dt, validate=False)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in idx:
        ops.gather_timeline(timeline, first, i, seq_len, -1, dt, validate=False)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / reps * 1e3
    nbytes = B * seq_len * frame * (4 + (4 if dt == torch.float32 else 2))
    print('vs_gather_timeline %s: %.1f us per batch of %d x %d frames, launch to launch on one stream  (%.0f GB/s read+write of %.1f MB)'
          % (dt, us, B, seq_len, nbytes / us / 1e3, nbytes / 1e6))

if '--skip_epochs' not in sys.argv:
    import taxibj_inputs  # noqa: E402
    tmp = tempfile.mkdtemp(prefix='taxibj_loader_bench_')
    try:
        tree = taxibj_inputs.write_tree(os.path.join(tmp, 'tree'))
        common = ['--device', '0', '--epochs', '24', '--batch_size', '32', '--num_workers', '0', '--seed', '3', '--log_interval', '6',
                  '--data', 'taxibj', '--architecture', 'vgg', '--nt_cond', '4', '--nt_pred', '4', '--offset', '4', '--precision', 'bf16']
        for name, extra in (('tree', ['--data_dir', tree]), ('synthetic', ['--data_dir', 'synthetic', '--synthetic_len', '192'])):
            cmd = [sys.executable, '-m', 'spatiotemporal_variable_separation_amd.main', '--xp_dir', os.path.join(tmp, 'xp_' + name)] + common + extra
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                print(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(r.returncode)
            fps = [float(m) for m in re.findall(r'\| (\d+) frames/s', r.stdout)]
            print('main --data taxibj on %-9s: %d epochs of 6 batches of 32 logged; median of the epochs after the first four %.0f frames/s '
                  '(min %.0f, max %.0f)' % (name, len(fps), np.median(fps[4:]), min(fps[4:]), max(fps[4:])))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

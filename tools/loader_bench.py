"""Throughput of the device-side batch assembly at the WaveEq recipe's sizes (README.md:90 of the reference: 64x64 frames, 5 + 20
frames per item, batch 128): one vs_gather_windows launch per batch from a [300, 300, 4096] fp32 set resident in HBM; and at the
chairs recipe's sizes (README.md:78: 64x64x3 frames, 5 + 10 frames per item, batch 128): one vs_chairs_gather launch per batch from a
[1184, 62, 64, 64, 3] uint8 set (the size of the train split), beside the host path it replaces -- PIL decoding the batch's 1920 PNG
files (written to a temporary directory; the files of a rendering are larger and slower to decode than these smooth images)."""
import os
import shutil
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spatiotemporal_variable_separation_amd import ops  # noqa: E402

n_seq, nt, frame, B, seq_len = 300, 300, 4096, 128, 25
data = torch.rand(n_seq, nt, frame, device='cuda')
per = nt + 1 - seq_len
g = torch.Generator().manual_seed(0)
for dt in (torch.float32, torch.bfloat16):
    idx = [torch.randint(0, n_seq * per, (B,), generator=g, dtype=torch.int32).cuda() for _ in range(20)]
    for i in idx[:3]:
        ops.gather_windows(data, i, per, seq_len, out_dtype=dt)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in idx:
        ops.gather_windows(data, i, per, seq_len, out_dtype=dt)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / len(idx) * 1e3
    nbytes = B * seq_len * frame * (4 + (4 if dt == torch.float32 else 2))
    print('%s: %.1f us per batch of %d x %d frames  (%.0f GB/s read+write, %.1f M frames/s)' % (dt, us, B, seq_len, nbytes / us / 1e3, B * seq_len / us))

# ---- chairs: one gather launch per batch against decoding the batch's PNG files on the host ------------------------------------------
n_obj, views, B, seq_len = 1184, 62, 128, 15
frames = torch.randint(0, 256, (n_obj, views, 64, 64, 3), dtype=torch.uint8, device='cuda')
for dt in (torch.float32, torch.bfloat16):
    descs = [torch.stack([torch.randint(0, n_obj, (B,), generator=g), torch.randint(0, views, (B,), generator=g)], dim=1).int().cuda()
             for _ in range(20)]
    for d in descs[:3]:
        ops.chairs_gather(frames, d, seq_len, dt, validate=False)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for d in descs:
        ops.chairs_gather(frames, d, seq_len, dt, validate=False)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / len(descs) * 1e3
    nbytes = B * seq_len * 64 * 64 * 3 * (1 + (4 if dt == torch.float32 else 2))
    print('chairs %s: %.1f us per batch of %d x %d frames  (%.0f GB/s read+write, %.1f M frames/s)'
          % (dt, us, B, seq_len, nbytes / us / 1e3, B * seq_len / us))

try:
    from PIL import Image
except ImportError:
    Image = None
if Image is None:
    print('chairs host path: PIL is not installed, not timed')
else:
    import numpy as np
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    import chairs_inputs  # noqa: E402
    tmp = tempfile.mkdtemp(prefix='loader_bench_chairs_')
    try:
        views_u8 = np.concatenate([chairs_inputs.object_views(k) for k in range(4)])
        names = []
        for i in range(B * seq_len):
            names.append(os.path.join(tmp, '%d.png' % i))
            Image.fromarray(views_u8[i % len(views_u8)], 'RGB').save(names[-1])
        for rep in range(2):                                   # the second pass reads from the page cache, like a second epoch
            t0 = time.perf_counter()
            batch = np.array([np.array(Image.open(f)) for f in names])
            x = torch.tensor(batch / 255).permute(0, 3, 1, 2).float()
            ms = (time.perf_counter() - t0) * 1e3
        print('chairs host path: %.1f ms per batch of %d PNG files decoded by PIL on one core (+ / 255, permute, float) -> %.0f us per file'
              % (ms, len(names), ms * 1e3 / len(names)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

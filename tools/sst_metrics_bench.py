"""SST evaluation metrics of one batch of 256 windows (10 days of 64 x 64), two ways, alternating, device events around each block:

  fused    ops.sst_frame_metrics: one vs_sst_frame_metrics launch on the normalised planes;
  unfused  torch broadcasting of the per-day constants into [256, 10, 10, 64, 64] forecasts and targets, the MSE by torch reductions, the
           rescale to the zone's range, then one vs_frame_metrics launch on the 25 600 plane pairs.

Both are warmed up, then ROUNDS blocks of REPS calls each are timed alternately; the median, minimum and maximum per call are printed, and
the largest difference between the two results.

    python tools/sst_metrics_bench.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spatiotemporal_variable_separation_amd import ops  # noqa: E402

B, T, H, W, ZONES, L, ROUNDS, REPS = 256, 10, 64, 64, 4, 365, 9, 40
g = torch.Generator().manual_seed(0)
target = torch.randn((B, T, H, W), generator=g).cuda()
pred = (target + 0.3 * torch.randn((B, T, H, W), generator=g).cuda()).contiguous()
consts = torch.stack([torch.rand(ZONES * L, generator=g) - 0.5, 0.5 + torch.rand(ZONES * L, generator=g),
                      10 + 10 * torch.rand(ZONES * L, generator=g), 0.6 + 0.8 * torch.rand(ZONES * L, generator=g)], dim=1).cuda()
zone = torch.randint(0, ZONES, (B,), generator=g).to(torch.int32).cuda()
day0 = (zone.cpu() * L + torch.randint(0, L - T, (B,), generator=g).to(torch.int32)).cuda()
zone_range = torch.tensor([[-4.0, 4.0]] * ZONES).cuda()


def fused():
    return ops.sst_frame_metrics(pred, target, consts, day0, zone, zone_range, validate=False)


def unfused():
    k = consts[day0.long()[:, None] + torch.arange(T, device='cuda')[None]]
    mn, sn, mc, sc = (k[:, None, :, i, None, None] for i in range(4))
    p = ((pred[:, :, None] * sn) + mn) * sc + mc
    t = ((target[:, :, None] * sn) + mn) * sc + mc
    mse = (p - t).pow(2).mean(dim=-1).mean(dim=-1).mean(dim=-1)
    lo, hi = zone_range[zone.long(), 0].view(-1, 1, 1, 1, 1), zone_range[zone.long(), 1].view(-1, 1, 1, 1, 1)
    _, ssim = ops.frame_metrics((p - lo) / (hi - lo), (t - lo) / (hi - lo), max_val=1.0)
    return mse, ssim


def block(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


for fn in (fused, unfused):
    for _ in range(5):
        fn()
torch.cuda.synchronize()
(mf, sf), (mu, su) = fused(), unfused()
print('largest relative MSE difference %.2e, largest SSIM difference %.2e' % (float((mf / mu - 1).abs().max()), float((sf - su).abs().max())))
times = {'fused': [], 'unfused': []}
for _ in range(ROUNDS):
    times['fused'].append(block(fused))
    times['unfused'].append(block(unfused))
for name, v in times.items():
    print('%-8s %8.1f us per batch of %d windows x %d days (median of %d blocks of %d calls; min %.1f, max %.1f)'
          % (name, float(np.median(v)), B, T, ROUNDS, REPS, min(v), max(v)))

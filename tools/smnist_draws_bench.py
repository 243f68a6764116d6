"""What the STOCHASTIC Moving-MNIST training data costs, host route against device route (VARSEP_MMNIST_DRAWS), on one MI355X:

  1. the trajectory launch alone at B = 128, two digits, 15 frames (vs_mmnist_stochastic_trajectories: draws and walks of 256 trajectories in one
     workgroup), beside `MovingMNIST.draw_stochastic(128)` on the same box's host (the Python loop the launch replaces), the upload of its
     tables, the render launch both routes share, and vs_mt19937_randint (the deterministic variant's draws) for scale; the kernel's
     registers, LDS and scratch from the compiler's resource report;
  2. loader + recorded DCGAN step in one process (the sizes of the recorded workload `mnist_b128`, bf16, B = 128): the step alone, with the
     host loader and with the device loader, alternating;
  3. `python -m spatiotemporal_variable_separation_amd.main --data mnist` on `synthetic_digits`, steps per second from its own log lines:
     deterministic data, and `--mnist_stochastic` with the variable at `host` and at `device`, alternating; `--parent DIR` adds the
     deterministic command run from a checkout of the parent commit (it needs its library built) as the baseline.

Every step that starts a process has its own time limit.  Writes the note given by --out.

    python tools/smnist_draws_bench.py [--out FILE] [--parent DIR] [--steps N]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]
import mmnist_draws_bench as base  # noqa: E402  (the helpers of the deterministic variant's tool: say, windows_us, host_ms)
from spatiotemporal_variable_separation_amd import _lib  # noqa: E402
from spatiotemporal_variable_separation_amd.configs import BASELINE_CONFIGS  # noqa: E402
from spatiotemporal_variable_separation_amd.data.moving_mnist import MovingMNIST  # noqa: E402
from spatiotemporal_variable_separation_amd.data.numpy_stream import DeviceRandomState  # noqa: E402

B, ND, T, SEED = 128, 2, 15, 3
HOST_CALLS = 20
REGIONS, REGION_STEPS = 4, 50
say = base.say


def resource_report(source, kernel):
    """{field: value} of `kernel` in csrc/`source` from hipcc's -Rpass-analysis=kernel-resource-usage, or None when there is no compiler."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    src = os.path.join(ROOT, 'spatiotemporal_variable_separation_amd', 'csrc', source)
    if not os.path.exists(hipcc):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Rpass-analysis=kernel-resource-usage', '-c', src, '-o',
                            os.path.join(tmp, 'x.o')], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        return None
    out, inside = {}, False
    for line in r.stderr.splitlines():
        m = re.search(r'remark:\s+(.*?)\s+\[-Rpass-analysis', line)
        if not m:
            continue
        text = m.group(1)
        if text.startswith('Function Name:'):
            inside = kernel in text
        elif inside and ':' in text:
            k, v = text.rsplit(':', 1)
            out[k.strip()] = v.strip()
    return out or None


def part_launch(ds, dev):
    say('## 1. The trajectory launch alone, B = %d, %d digits, %d frames (%d trajectories), against the host route' % (B, ND, T, B * ND))
    say()
    s, room = ds.max_speed, ds.frame_size - ds.digit_shape[0]
    lows, highs = (0, 0, 0, -s, -s), (ds.n_source, room + 1, room + 1, s + 1, s + 1)
    stream = DeviceRandomState(np.random.RandomState(SEED), dev)
    ds.rng = np.random.RandomState(SEED)
    desc, positions = ds.draw_stochastic(B)
    ds.rng = DeviceRandomState(np.random.RandomState(SEED), dev)
    dev_desc, dev_positions = ds.draw_stochastic(B)
    same = np.array_equal(dev_desc.cpu().numpy(), desc) and np.array_equal(dev_positions.cpu().numpy(), positions)
    walk = base.windows_us(lambda: stream.stochastic_trajectories(B * ND, T, lows, highs, room, room, s, desc_nd=ND))
    draws = base.windows_us(lambda: stream.randint_table(lows, highs, B * ND))
    render = base.windows_us(lambda: ds.render_stochastic(dev_desc, dev_positions))
    enqueue_ms = 1e3 * base._enqueue_s(lambda: stream.stochastic_trajectories(B * ND, T, lows, highs, room, room, s, desc_nd=ND))
    ds.rng = np.random.RandomState(SEED)
    t0 = time.perf_counter()
    for _ in range(HOST_CALLS):
        ds.draw_stochastic(B)
    host_draw_ms = 1e3 * (time.perf_counter() - t0) / HOST_CALLS
    count = np.random.RandomState(SEED)                      # a fresh stream stands at pos 624: its first draw makes block 1
    blocks, before = 0, count.get_state()[1].copy()
    ds.rng = count
    for _ in range(B):                                       # (one item consumes far less than a block)
        ds.draw_stochastic(1)
        now = count.get_state()[1]
        if not np.array_equal(now, before):
            blocks, before = blocks + 1, now.copy()
    outputs = (blocks - 1) * 624 + count.get_state()[2]
    upload_ms = base.host_ms(lambda: (torch.from_numpy(desc).to(dev, non_blocking=True), torch.from_numpy(positions).to(dev, non_blocking=True)))
    say('| what | time | how measured |')
    say('|---|---|---|')
    say('| `vs_mmnist_stochastic_trajectories`, one launch (one workgroup of 1024 lanes, the speculative form) | **%.1f us** (%.1f - %.1f) | median '
        '(min - max) per launch over %d windows of %d launches between two events, warm |' % (walk + (base.REPS, base.LAUNCHES)))
    say('| `vs_mt19937_randint`, the deterministic variant\'s draws for the same batch, in this run | %.1f us (%.1f - %.1f) | as the first row |' % draws)
    say('| host time to enqueue the trajectory launch (`DeviceRandomState.stochastic_trajectories`) | %.3f ms | wall clock, mean of %d calls, no '
        'synchronise inside the window |' % (enqueue_ms, 2000))
    say('| `MovingMNIST.draw_stochastic(%d)` on the host (the Python loop: draws and walks) | **%.2f ms** (%.1f us per trajectory) | wall clock, mean '
        'of %d calls, this box, this run |' % (B, host_draw_ms, 1e3 * host_draw_ms / (B * ND), HOST_CALLS))
    say('| upload of its desc and positions tables, which the device route removes | %.3f ms | wall clock, mean of %d calls, one synchronise at '
        'the end |' % (upload_ms, base.HOST_CALLS))
    say('| `vs_moving_mnist_place` (the render both routes share), fp32 out | %.1f us (%.1f - %.1f) | as the first row |' % render)
    say()
    say('* The device tables equal the host loop\'s for the same seed: %s.  One batch consumes %d outputs of the stream (%.2f per trajectory) and '
        'crosses %d block regenerations.' % (same, outputs, outputs / (B * ND), blocks))
    say('* The launch takes %.1f us where the host route takes %.0f us on this box (%.0fx), and %.1fx the %.1f us of `vs_mt19937_randint` '
        '(recorded for the deterministic variant: 29.1 us).' % (walk[0], 1e3 * host_draw_ms, 1e3 * host_draw_ms / walk[0], walk[0] / draws[0], draws[0]))
    rep = resource_report('vs_mmnist_walk.hip', 'mmnist_walk_kernel')
    if rep is None:
        say('* Compiler resource report: not measured (no hipcc on this box).')
    else:
        say('* Compiler resource report of the kernel (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): VGPRs %s, AGPRs %s, SGPRs %s, scratch '
            '%s bytes/lane, LDS %s bytes/block, occupancy %s waves/SIMD.' % (rep.get('VGPRs'), rep.get('AGPRs'), rep.get('TotalSGPRs'),
                                                                             rep.get('ScratchSize [bytes/lane]'), rep.get('LDS Size [bytes/block]'),
                                                                             rep.get('Occupancy [waves/SIMD]')))
    say()
    return walk


def part_step(ds, dev, walk):
    from spatiotemporal_variable_separation_amd import functional as VF
    from spatiotemporal_variable_separation_amd.networks.factory import build_sep_net
    from spatiotemporal_variable_separation_amd.optim import Adam
    from spatiotemporal_variable_separation_amd.train import GraphedStep, enable_fused_update, enable_update_in_backward
    cfg = dict(BASELINE_CONFIGS['mnist_b128'])
    say('## 2. Loader + recorded step in one process (`mnist_b128`: DCGAN, bf16, B = %d, nt_cond %d, nt_pred %d), stochastic data, the routes '
        'alternating' % (cfg['batch'], cfg['nt_cond'], cfg['nt_pred']))
    say()
    torch.manual_seed(1234)
    np.random.seed(1234)
    net = build_sep_net(cfg).to(dev)
    net.train()
    opt = Adam(net.parameters(), lr=4e-4, betas=(0.9, 0.99))
    VF.set_precision('bf16')
    enable_update_in_backward(opt, net, None, scaler=None)
    enable_fused_update(opt, net, None, None)
    VF.fold_repeated_gradients(True)
    lam = cfg['lambdas']
    rngs = {'host': np.random.RandomState(SEED + 7919), 'device': DeviceRandomState(np.random.RandomState(SEED + 7919), dev)}
    ds.rng = rngs['host']
    cond, target = ds.batch(B)
    graphed = GraphedStep(net, opt, cond, target, cfg['nt_cond'], cfg['nt_pred'], cfg['offset'], (lam['ae'], lam['s'], lam['t'], lam['pred']),
                          bool(cfg.get('average_tloss')), warmup=3)
    for route in ('host', 'device'):
        ds.rng = rngs[route]
        for _ in range(10):
            graphed.step(*ds.batch(B))
    torch.cuda.synchronize()
    rows = {'host': [], 'device': [], 'step only': []}
    for region in range(REGIONS):
        for route in ('host', 'device', 'step only'):
            ds.rng = rngs.get(route)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            loader_s = 0.0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(REGION_STEPS):
                if route == 'step only':
                    graphed.step()
                    continue
                t1 = time.perf_counter()
                batch = ds.batch(B)
                loader_s += time.perf_counter() - t1
                graphed.step(*batch)
            e1.record()
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            rows[route].append((e0.elapsed_time(e1) / REGION_STEPS, 1e3 * wall / REGION_STEPS, 1e3 * loader_s / REGION_STEPS))
    say('| route | device time per step, events round loader + step: median (min - max) | wall clock per step | host time inside the loader call '
        'per step |')
    say('|---|---|---|---|')
    med = {}
    for route in ('host', 'device', 'step only'):
        ev, wall, load = (np.array(x) for x in zip(*rows[route]))
        med[route] = (float(np.median(ev)), float(np.median(wall)), float(np.median(load)))
        say('| %s | %.3f ms (%.3f - %.3f) | %.3f ms | %s |' % (
            'VARSEP_MMNIST_DRAWS=' + route if route != 'step only' else 'the recorded step alone, replayed on the last batch (no loader)',
            med[route][0], ev.min(), ev.max(), med[route][1], '%.3f ms' % med[route][2] if route != 'step only' else '-'))
    say()
    say('* %d regions of %d steps per route, in the order host, device, step alone, repeated.' % (REGIONS, REGION_STEPS))
    say('* Device route minus the step alone, device time per step: %+.1f us; the trajectory launch alone takes %.1f us.'
        % (1e3 * (med['device'][0] - med['step only'][0]), walk[0]))
    bound = med['host'][1] > 1.05 * med['step only'][0]
    say('* Host route: wall clock per step %.3f ms against %.3f ms for the recorded step alone on the device -- the host route %s host-bound on '
        'this box (%.2fx the step).  The device route: %.3f ms wall clock per step; it frees %.3f ms of host time per step (loader call: %.3f ms -> '
        '%.3f ms).' % (med['host'][1], med['step only'][0], 'IS' if bound else 'is NOT', med['host'][1] / med['step only'][0], med['device'][1],
                       med['host'][2] - med['device'][2], med['host'][2], med['device'][2]))
    say()
    del graphed, net, opt


def run_main(cwd, stochastic, draws, steps, tmp, tag):
    """Steps per second from main's own log lines (the first of them, which holds the recording, dropped)."""
    xp = os.path.join(tmp, tag)
    cmd = [sys.executable, '-m', 'spatiotemporal_variable_separation_amd.main', '--xp_dir', xp, '--data_dir', 'synthetic_digits', '--data', 'mnist',
           '--device', '0', '--epochs', '1', '--batch_size', str(B), '--num_workers', '0', '--seed', str(SEED), '--log_interval', '50',
           '--precision', 'bf16'] + (['--mnist_stochastic'] if stochastic else [])
    env = dict(os.environ, VARSEP_MMNIST_EPOCH_LEN=str(B * steps))
    env.pop('VARSEP_MMNIST_DRAWS', None)
    if draws is not None:
        env['VARSEP_MMNIST_DRAWS'] = draws
    t0 = time.perf_counter()
    r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=420)
    if r.returncode != 0:
        raise RuntimeError('main failed (%d) in %s:\n%s' % (r.returncode, cwd, (r.stdout[-1500:] + r.stderr[-3000:])))
    fps = [float(m) for m in re.findall(r'\| (\d+) frames/s', r.stdout)]
    per_s = [f / (B * 10) for f in fps[1:]]
    return per_s, time.perf_counter() - t0


def part_main(parent, steps):
    say('## 3. `python -m spatiotemporal_variable_separation_amd.main --data mnist --data_dir synthetic_digits --precision bf16 --batch_size %d`' % B)
    say()
    say('Steps per second from the command\'s own log lines (`--log_interval 50`: wall clock between two lines, each after a synchronise), %d steps '
        'per run, the first line (it holds the recording of the step) dropped; one process per run, the runs alternating.' % steps)
    say()
    say('| run | tree | data | VARSEP_MMNIST_DRAWS | steps/s: median (min - max) over the log lines | ms per step | whole process |')
    say('|---|---|---|---|---|---|---|')
    order = ([('parent', False, None)] if parent else []) + [('this', False, None), ('this', True, 'host'), ('this', True, 'device')]
    with tempfile.TemporaryDirectory() as tmp:
        n = 0
        for rep in range(2):
            for tree, stochastic, draws in order:
                n += 1
                per_s, total = run_main(parent if tree == 'parent' else ROOT, stochastic, draws, steps, tmp, 'run%d' % n)
                med = float(np.median(per_s))
                say('| %d | %s | %s | %s | %.1f (%.1f - %.1f) | %.3f | %.1f s |' % (
                    n, 'parent commit' if tree == 'parent' else 'this change', '`--mnist_stochastic`' if stochastic else 'deterministic',
                    draws or '(unset: host)', med, min(per_s), max(per_s), 1e3 / med, total))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'smnist_draws_timing.md'))
    ap.add_argument('--parent', default=None, help='a checkout of the parent commit with its library built: the baseline of part 3')
    ap.add_argument('--steps', type=int, default=300, help='steps per run of part 3')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    _lib.load_library()
    say('# The stochastic Moving-MNIST training data, host route against device route (one MI355X, `tools/smnist_draws_bench.py`)')
    say()
    say('NumPy %s.  Device times come from HIP events, host times from the wall clock on the same box in the same run.  The kernel form that '
        'ships is the SPECULATIVE one (csrc/vs_mmnist_walk_core.h, `vsw_walk_lanes`: window of four blocks in LDS, a walk from every offset, '
        'pointer-doubling chase, second walk that stores); the one-lane form is the host build\'s checker.' % np.__version__)
    say()
    try:
        ds = MovingMNIST.make_dataset('synthetic_digits', 64, 5, T, 4, False, ND, True, device=dev, seed=SEED)
        walk = part_launch(ds, dev)
        part_step(ds, dev, walk)
        del ds
        torch.cuda.empty_cache()
        part_main(os.path.abspath(args.parent) if args.parent else None, args.steps)
    finally:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(base.lines) + '\n')


if __name__ == '__main__':
    main()

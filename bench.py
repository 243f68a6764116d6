"""Headline benchmark: training frames/s of the var_sep hot path on MI355X (contract in the task statement).

    python bench.py --gpus N --steps K --warmup W [--config waveeq] [--precision bf16|fp16|fp32] [--dump-outputs DIR] [--full]

One step = ae_loss + zero_order_loss + get_forecast + forecast MSE + t-regulariser, backward, gradient all-reduce
(N > 1) and the Adam update, on one seeded synthetic batch per rank that is resident in HBM before timing starts.
`value` = N * batch * nt_pred / step time (whole-job predicted frames per second).  Default workload = BASELINE.json
configs[1] (WaveEq MLP, bf16), the configuration the metric is quoted on that fits one GPU.

Ranks: under `torch.distributed.run` (RANK / WORLD_SIZE in the environment) this process IS one rank.  Started plainly with
`--gpus N` (N > 1) it launches N rank processes itself -- before anything touches the GPU -- one per device over RCCL, and
rank 0 prints the JSON line.  VARSEP_BENCH_SHARE_GPU=1 puts every rank on cuda:0 and exchanges gradients over gloo (the
one-GPU test of the N > 1 path, tests/test_safety_gpu.py::test_bench_spawns_its_own_ranks).

Timing: W warm-up steps, then `--repeats` timed regions of EXACTLY K steps each, every region bracketed by
barrier + torch.cuda.synchronize() on both sides and reduced with MAX over ranks; the reported ms_per_step is the median region
(all of them are listed in `ms_per_step_all`).  A plain run times ONE region (K timed steps in all) and does nothing else: no profiler
passes, no instrumented eager steps, no further workloads, no CPU baseline.  `--full` (default 5 regions, extended to
VARSEP_BENCH_MIN_TIMED_S of timed time) adds everything below.

`--dump-outputs DIR`: after the timed steps, what the LAST timed step handed its caller is written as DIR/<name>.npy -- loss.npy (the
total loss the step returns, float64 [1]) and state.npy (the parameters and BatchNorm statistics the step leaves, float32: every
floating-point entry of the network's state_dict flattened in state_dict order, a fixed seeded sample of DUMP_MAX_ELEMS of them when
larger); with --eval, forecast.npy (the last get_forecast output, same sampling).  Inputs are seeded: the same arguments give the same
inputs in every run.

With `--full` the line also carries `configs`: further BASELINE workloads timed the same way with fewer steps, each with the roofline
position of its dominant kernel group -- at N = 1 Moving-MNIST DCGAN B=128, TaxiBJ VGG B=100, SST nt_pred 40 B=8 in bf16 and SST in fp16 (the dtype
BASELINE.json configs[4] states); at N > 1 TaxiBJ and SST (configs[3], configs[4]: the two workloads stated at 8 GPUs), data-parallel
over the same ranks.

`roofline`: kernel GROUPS (spatiotemporal_variable_separation_amd/profiling.py).  Algorithmic FLOPs / bytes per step are accounted live.
The duration of a group inside the REPLAYED step is measured IN THIS RUN: before this process touches the GPU it runs the same command
(same workload, steps, warm-up; VARSEP_BENCH_NO_EVENTS=1) as a child under `rocprofv3 --kernel-trace --stats` and reads the kernel
statistics (`timing: "replay-live"`) -- HIP events cannot be recorded inside a hipGraph replay (tools/graph_event_probe.py: they read 4.7 us
around a 4096^3 GEMM).  Fallbacks, in order: the committed table profiles/r<NN>_<workload>_<dtype>_replay.json when its `_source_sha` still
equals profiling.source_sha() (`"replay-committed"`); live HIP events around every launch of three eager steps (`"eager"`, with
`"stale": true` when a committed table exists but belongs to other sources).  VARSEP_BENCH_LIVE_PROFILE=0 | headline | all (default all).

Output: stdout carries ONE JSON line of < 4 KB (headline; with `--full` also one roofline object, cpu_baseline, one short entry per
further workload); everything else (all regions, every group's roofline, eager-event figures, traffic sources, prose) goes to
`bench_detail.json` next to this file and to stderr.
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import spatiotemporal_variable_separation_amd  # noqa: E402

spatiotemporal_variable_separation_amd.configure_single_gpu_queues()   # HIP runtime queue knobs: before anything initialises HIP

import numpy as np          # noqa: E402
import torch                # noqa: E402

EXTRA_DEFAULT = 'mnist_b128,taxibj,sst,sst_fp16'
EXTRA_DEFAULT_DIST = 'taxibj,sst'          # N > 1: the two workloads BASELINE.json states at 8 GPUs (configs[3], configs[4])
EXTRA_STEPS = {'mnist_b128': (10, 3), 'taxibj': (8, 3), 'sst': (3, 2), 'sst_fp16': (3, 2), 'mnist_b16': (10, 3), 'chairs': (6, 2), 'waveeq': (20, 5)}


def split_workload(name, default_precision):
    """'sst_fp16' -> ('sst', 'fp16'): a workload name may carry the compute type BASELINE.json states for it (configs[4]: SST in fp16)."""
    for suffix in ('fp16', 'bf16', 'fp32'):
        if name.endswith('_' + suffix):
            return name[:-len(suffix) - 1], suffix
    return name, default_precision


def parse():
    p = argparse.ArgumentParser()
    p.add_argument('--gpus', type=int, default=1)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--repeats', type=int, default=None, help='timed regions of --steps steps each; the median is reported (default: 1, '
                   'with --full 5)')
    p.add_argument('--full', action='store_true', help='also measure what the headline does not need: profiler passes of the replayed '
                   'step, per-kernel-group rooflines, the further workloads under "configs", the CPU baseline, at least '
                   'VARSEP_BENCH_MIN_TIMED_S of timed regions')
    p.add_argument('--dump-outputs', dest='dump_outputs', default=None, metavar='DIR',
                   help='write what the last timed step computed as DIR/<name>.npy (loss.npy, state.npy; --eval: forecast.npy)')
    p.add_argument('--config', default='waveeq')
    p.add_argument('--precision', default='bf16', choices=['bf16', 'fp16', 'fp32'])
    p.add_argument('--batch', type=int, default=None, help='per-GPU batch (default: the config\'s)')
    p.add_argument('--eval', action='store_true', dest='eval_mode',
                   help='time the inference path instead of the training step: `sep_net.eval(); get_forecast(cond, nt_cond + --horizon)` under '
                        'no_grad, BatchNorm folded into the convolutions (what the reference\'s test/*/test.py run)')
    p.add_argument('--horizon', type=int, default=95, help='--eval: predicted frames beyond the conditioning window (README.md:116: 95)')
    p.add_argument('--no_cpu_baseline', action='store_true')
    p.add_argument('--no_graph', action='store_true', help='issue every kernel from Python instead of replaying a hipGraph')
    p.add_argument('--graph_stats', action='store_true', help='count the nodes / edges of the recorded step (keeps the captured hipGraph_t) and write '
                   'them to gpurun_out/graph_stats.json')
    p.add_argument('--cpu_steps', type=int, default=None)
    p.add_argument('--extra_configs', default=None,
                   help='comma list of further workloads appended under "configs" (default with --full at N=1 with the default workload: '
                        + EXTRA_DEFAULT + '; "none" disables)')
    args = p.parse_args()
    if args.repeats is None:
        args.repeats = 5 if args.full else 1
    return args


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def spawn_ranks(args):
    """`python bench.py --gpus N` outside a launcher: start N rank processes (children of this one, which never touches the GPU:
    torch.cuda.device_count() does not initialise it) and exit with the worst return code.  Rank 0 inherits stdout."""
    n = args.gpus
    share = os.environ.get('VARSEP_BENCH_SHARE_GPU') == '1'
    have = torch.cuda.device_count()
    if have < n and not share:
        sys.stderr.write(f'bench.py: --gpus {n} but only {have} device(s) visible (VARSEP_BENCH_SHARE_GPU=1 shares cuda:0 over gloo)\n')
        sys.exit(2)
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        for k in env.pop('VARSEP_PACKAGE_SET', '').split():     # single-GPU runtime knobs the package set in THIS process
            env.pop(k, None)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else sys.stderr))
    rcs = [p.wait() for p in procs]
    sys.exit(max(abs(rc) for rc in rcs))


def physical_cores():
    """Physical cores of the host: distinct (package, core) pairs of /proc/cpuinfo, else half the logical CPUs when SMT siblings show."""
    try:
        seen, pkg = set(), None
        for ln in open('/proc/cpuinfo'):
            if ln.startswith('physical id'):
                pkg = ln.split(':')[1].strip()
            elif ln.startswith('core id'):
                seen.add((pkg, ln.split(':')[1].strip()))
        if seen:
            return max(1, len(seen))
    except OSError:
        pass
    return max(1, os.cpu_count() or 1)


def cpu_baseline(cfg, steps):
    """Time the CPU oracle (plain PyTorch fp32 restatement of the reference) on the host cores, same workload."""
    from oracle import cpu_ref
    from spatiotemporal_variable_separation_amd.data.synthetic import synthetic_batch
    torch.manual_seed(1234)
    np.random.seed(1234)
    ocfg = dict(cfg)
    net = cpu_ref.build_sep_net(ocfg)
    net.train()
    cond, target = synthetic_batch(cfg['data'], cfg['batch'], cfg['nt_cond'], cfg['nt_pred'], seed=1234)
    lam = cfg['lambdas']
    opt = torch.optim.Adam(net.parameters(), lr=4e-4, betas=(0.9, 0.99))

    def step():
        opt.zero_grad()
        total, _, _, _ = cpu_ref.training_losses(cond, target, net, cfg['nt_cond'], cfg['nt_pred'], cfg['offset'],
                                                 cfg.get('skipco', False), lam['ae'], lam['s'], lam['t'], lam['pred'],
                                                 average_tloss=bool(cfg.get('average_tloss')))
        total.backward()
        opt.step()
    # thread counts: 8 (comparable with the survey container), 16, 32 and all physical cores of the host; the best one is
    # reported.  A count whose warm-up step alone takes 2.5 x the best step so far is recorded from that one step and not timed further (128
    # threads on this 256 x 20480-row problem: 3-3.7 s per step of thread hand-over against 0.65 s on 8 -- VERDICT round 5, weak item 9)
    default_threads = torch.get_num_threads()
    tried = {}
    for nthr in sorted({8, 16, 32, physical_cores()}):
        torch.set_num_threads(nthr)
        t0 = time.time()
        step()
        warm = time.time() - t0
        if tried and warm > 2.5 * min(tried.values()):
            tried[nthr] = warm
            continue
        t0 = time.time()
        for _ in range(steps):
            step()
        tried[nthr] = (time.time() - t0) / steps
    torch.set_num_threads(default_threads)
    nthr, dt = min(tried.items(), key=lambda kv: kv[1])
    return {'value': round(cfg['batch'] * cfg['nt_pred'] / dt, 1), 'unit': 'frames/s', 'cores': nthr,
            'threads_8': {'value': round(cfg['batch'] * cfg['nt_pred'] / tried[8], 1), 'ms_per_step': round(tried[8] * 1e3, 1),
                          'note': 'torch.set_num_threads(8): comparable with the survey container figures of BASELINE.md section 2'},
            'by_threads_ms_per_step': {str(k): round(v * 1e3, 1) for k, v in tried.items()}, 'logical_cpus': os.cpu_count(),
            'physical_cores': physical_cores(),
            'kind': 'port', 'sample': f'{steps} full training steps of the same workload (batch {cfg["batch"]}, fp32, CPU '
            f'oracle = plain-PyTorch restatement of the reference) after 1 warm-up, best of thread counts '
            f'{ {k: round(v * 1e3) for k, v in tried.items()} } ms/step on {physical_cores()} physical cores / {os.cpu_count()} logical CPUs',
            'ms_per_step': round(dt * 1e3, 1)}


class Ranks:
    """Process-group facts of this rank (one process per GPU)."""

    def __init__(self, args):
        self.rank = int(os.environ.get('RANK', 0))
        self.world = int(os.environ.get('WORLD_SIZE', 1))
        self.share = os.environ.get('VARSEP_BENCH_SHARE_GPU') == '1'
        local = 0 if self.share else int(os.environ.get('LOCAL_RANK', 0))
        torch.cuda.set_device(local)
        self.dev = torch.device('cuda', local)
        # VARSEP_BENCH_FORCE_DIST=1 runs the data-parallel code path (process group, flat buckets, RCCL all-reduce per step)
        # at world size 1, so the N>1 path can be exercised on a one-GPU box
        self.ddp = self.world > 1 or os.environ.get('VARSEP_BENCH_FORCE_DIST') == '1'
        self.backend = None
        if self.ddp:
            import torch.distributed as dist
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            os.environ.setdefault('MASTER_PORT', '29511')
            self.backend = 'gloo' if self.share else 'nccl'
            if self.backend == 'nccl':
                dist.init_process_group('nccl', device_id=self.dev, rank=self.rank, world_size=self.world)
            else:
                dist.init_process_group('gloo', rank=self.rank, world_size=self.world)
        if self.world != args.gpus and self.rank == 0:
            sys.stderr.write(f'bench.py: --gpus {args.gpus} but WORLD_SIZE={self.world}: reporting the {self.world} rank(s) that run\n')

    def barrier(self):
        if self.ddp:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(self, x):
        if not self.ddp:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=self.dev if self.backend == 'nccl' else 'cpu')
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        return t.item()

    def close(self):
        if self.ddp:
            torch.distributed.destroy_process_group()


class ExchangeTimeout(RuntimeError):
    pass


DUMP_MAX_ELEMS = 1 << 22           # elements per array written by --dump-outputs: 16 MB of float32 (the arrays of one run stay under 64 MB)


def _flat_sample(tensors, seed=1234):
    """The tensors' elements, flattened and concatenated in order, as float32; above DUMP_MAX_ELEMS a fixed sample of DUMP_MAX_ELEMS of them
    (sorted positions drawn by numpy.random.default_rng(seed), which leaves the global NumPy stream alone: the same positions in every run
    of the same workload)."""
    sizes = [t.numel() for t in tensors]
    total = sum(sizes)
    if total <= DUMP_MAX_ELEMS:
        return np.concatenate([t.detach().reshape(-1).float().cpu().numpy() for t in tensors] or [np.zeros(0, np.float32)])
    pos = np.sort(np.random.default_rng(seed).integers(0, total, size=DUMP_MAX_ELEMS))
    out, off = [], 0
    for t, n in zip(tensors, sizes):
        lo, hi = np.searchsorted(pos, [off, off + n])
        if hi > lo:
            idx = torch.from_numpy(pos[lo:hi] - off).to(t.device)
            out.append(t.detach().reshape(-1).index_select(0, idx).float().cpu().numpy())
        off += n
    return np.concatenate(out)


def dump_training_outputs(dump_dir, rk, net, opt, sync, loss):
    """--dump-outputs of a training workload, right after the last timed step: the total loss that step returned (loss.npy) and the state
    it left (state.npy: every floating-point entry of the network's state_dict -- parameters, BatchNorm statistics -- in state_dict order)."""
    if sync is not None and getattr(sync, 'masters_dirty', False):
        sync.sync_masters(opt)               # sharded optimizer: every rank's slice of the fp32 masters (a collective: every rank is here)
    if rk.rank != 0:
        return
    torch.cuda.synchronize()
    os.makedirs(dump_dir, exist_ok=True)
    np.save(os.path.join(dump_dir, 'loss.npy'), np.array([float(loss.item())], dtype=np.float64))
    np.save(os.path.join(dump_dir, 'state.npy'), _flat_sample([v for v in net.state_dict().values() if v.is_floating_point()]))


def run_workload(name, args, rk, steps, warmup, repeats, batch=None, precision=None, dump_dir=None):
    """`_run_workload`; if the integrator's inter-workgroup exchange reports a time-out while it runs in its XCD-local form (a slab's ring of
    workgroups is assumed to share an XCD, csrc/vs_rollout.hip), the workload is measured again with the placement-independent agent-scope
    exchange instead of failing the run (every rank takes the same decision: the flag is all-reduced)."""
    try:
        return _run_workload(name, args, rk, steps, warmup, repeats, batch=batch, precision=precision, dump_dir=dump_dir)
    except ExchangeTimeout as e:
        if os.environ.get('VS_ROLLOUT_XCD_LOCAL', '1') == '0':
            raise
        if rk.rank == 0:
            print('bench.py: %s -- measuring again with VS_ROLLOUT_XCD_LOCAL=0' % e, file=sys.stderr)
        os.environ['VS_ROLLOUT_XCD_LOCAL'] = '0'
        return _run_workload(name, args, rk, steps, warmup, repeats, batch=batch, precision=precision, dump_dir=dump_dir)


def _run_workload(name, args, rk, steps, warmup, repeats, batch=None, precision=None, dump_dir=None):
    """Build the workload `name`, warm up, time `repeats` regions of `steps` steps; returns timings + (--full) per-kernel event profile.
    `dump_dir`: write what the last timed step computed there (dump_training_outputs)."""
    precision = precision or args.precision
    from spatiotemporal_variable_separation_amd import functional as VF, ops
    from spatiotemporal_variable_separation_amd.configs import BASELINE_CONFIGS
    from spatiotemporal_variable_separation_amd.data.synthetic import synthetic_batch
    from spatiotemporal_variable_separation_amd.networks.factory import build_sep_net
    from spatiotemporal_variable_separation_amd.optim import Adam
    from spatiotemporal_variable_separation_amd.parallel import GradAllReducer, broadcast_module_state
    from spatiotemporal_variable_separation_amd.train import (GraphedStep, chain_weight_parameters, compute_losses,
                                                               enable_fused_update, enable_update_in_backward, make_loss_scaler)
    dev = rk.dev
    cfg = dict(BASELINE_CONFIGS[name])
    if batch:
        cfg['batch'] = batch
    torch.manual_seed(1234)
    np.random.seed(1234)                     # same t_random sequence on every rank
    net = build_sep_net(cfg).to(dev)
    net.train()
    if rk.ddp:
        broadcast_module_state(net)
    # Wire format of the gradient all-reduce (reported in config.grad_allreduce; VARSEP_GRAD_COMM=fp32 | bf16 overrides).  SURVEY 8e's
    # contract is fp32 buckets (N replicas == the single-process step on the concatenated batch); the conv families keep it -- 102 / 63 MB
    # per step against 12 / 23 ms of compute.  The WaveEq MLP's 243 MB would cost more on the wire than its 1.4 ms step, so in bf16 mode
    # its gradients travel as bf16 (a stated deviation: the chains' weight-gradient GEMMs write the wire image themselves).
    from spatiotemporal_variable_separation_amd.train import _mlp_family as _is_mlp
    comm_default = 'bf16' if (precision == 'bf16' and _is_mlp(net)) else 'fp32'
    comm_bf16 = precision == 'bf16' and os.environ.get('VARSEP_GRAD_COMM', comm_default) == 'bf16'
    direct = chain_weight_parameters(net) if (comm_bf16 and os.environ.get('VARSEP_GRAD_DIRECT_LOWP', '1') == '1') else None
    # conv families: the decoder's gradients (complete first in backward) in leading buckets of their own -- the recorded step is split
    # there and their all-reduce travels beside the integrator's / encoders' backward kernels (train.GraphedStep.segmented)
    early = None if _is_mlp(net) else list(net.decoder.parameters())
    from spatiotemporal_variable_separation_amd.train import rollout_weight_stacks, shard_optimizer_default
    use_graph_planned = (not args.no_graph) and os.environ.get('VARSEP_BENCH_GRAPH_ALL', '1') == '1'
    shard = bool(direct) and use_graph_planned and precision == 'bf16' and shard_optimizer_default()
    sync = GradAllReducer(net.parameters(), force=(rk.world == 1), comm_dtype=torch.bfloat16 if comm_bf16 else torch.float32,
                          lowp_direct=direct, early=early, shard_direct=shard, stacked=rollout_weight_stacks(net)) if rk.ddp else None
    use_graph = (not args.no_graph) and os.environ.get('VARSEP_BENCH_GRAPH_ALL', '1') == '1'
    opt = Adam(net.parameters(), lr=4e-4, betas=(0.9, 0.99))
    cond, target = synthetic_batch(cfg['data'], cfg['batch'], cfg['nt_cond'], cfg['nt_pred'], device=dev, seed=1234 + rk.rank)
    lam = cfg['lambdas']
    VF.set_precision(precision)
    scaler = make_loss_scaler(dev) if precision == 'fp16' else None     # reference train.py:96-97: GradScaler with fp16 autocast
    enable_update_in_backward(opt, net, sync, scaler=scaler)
    if precision != 'fp32':
        enable_fused_update(opt, net, sync, scaler)      # (GraphedStep does the same; here for --no_graph and the instrumented eager steps)
    # conv families under a reducer: convolution / BatchNorm gradients accumulate straight into the bucket views, folding stays on
    from spatiotemporal_variable_separation_amd.train import _mlp_family, conv_gradient_sinks
    conv_sinks = conv_gradient_sinks(net, sync) if (sync is not None and not _mlp_family(net)) else None
    VF.fold_repeated_gradients(os.environ.get('VARSEP_FOLD_GRADS', '1') == '1' and (sync is None or bool(conv_sinks)))

    def step():
        if sync is not None:
            sync.zero_grad()
            VF.set_conv_grad_outputs(conv_sinks)
        else:
            opt.zero_grad(set_to_none=True)
        total, _, _, _ = compute_losses(cond, target, net, cfg['nt_cond'], cfg['nt_pred'], cfg['offset'],
                                        cfg.get('skipco', False), lam['ae'], lam['s'], lam['t'], lam['pred'],
                                        average_tloss=bool(cfg.get('average_tloss')))
        if scaler is not None:
            scaler.backward(total)
        else:
            total.backward()
        VF.set_conv_grad_outputs(None)
        if sync is not None:
            sync.all_reduce()
        if scaler is not None:
            scaler.step(opt)
        else:
            opt.step()
        VF.flush_bn_call_counts()
        return total

    graphed = None
    graph_stats = None
    if use_graph:
        # the timed region replays the recorded step (train.GraphedStep: the same kernels, launched by hipGraphLaunch instead
        # of Python-issued launches); with N > 1 ranks: graph(losses + backward) -> bucket all-reduces -> graph(Adam)
        # node / edge counts of the recording: only on request (`--graph_stats` sets VARSEP_GRAPH_STATS=1 for this process: the captured hipGraph_t
        # is then kept, torch.cuda.CUDAGraph(keep_graph=True) -- a different capture path inside torch, so never in a default run); a default run
        # quotes the committed table profiles/rNN_graph_stats.json while its source hash matches
        graphed = GraphedStep(net, opt, cond, target, cfg['nt_cond'], cfg['nt_pred'], cfg['offset'],
                              (lam['ae'], lam['s'], lam['t'], lam['pred']), bool(cfg.get('average_tloss')),
                              warmup=max(1, min(warmup, 3)), grad_sync=sync, scaler=scaler)
        timed_step = graphed.step
        try:
            graph_stats = graphed.graph_stats()
        except Exception:                                 # measurement only: never in the way of the timing
            graph_stats = None
    else:
        timed_step = step
    for _ in range(warmup):
        timed_step()
    events_on = args.full and os.environ.get('VARSEP_BENCH_NO_EVENTS') is None
    n_inst = 3                                # instrumented eager steps after a graph-replay timed region
    ops.profile_reset(enable=False)
    regions = []
    loss = None
    # regions of EXACTLY `steps` steps each; beyond the `repeats` asked for, further regions are added until the timed regions sum to
    # VARSEP_BENCH_MIN_TIMED_S (default 1 s; the headline's 20-step regions are ~25 ms: five of them are too coarse for 1 % statements), at
    # most 200.  The decision uses the MAX-over-ranks clock every rank holds, so all ranks run the same number of regions.
    min_timed = float(os.environ.get('VARSEP_BENCH_MIN_TIMED_S', '1.0')) if graphed is not None and events_on else 0.0
    rep = -1
    while True:
        rep += 1
        if rep >= max(1, repeats) and (sum(regions) >= min_timed or rep >= 200):
            break
        if graphed is None and events_on and rep == 0:
            # eager loop: HIP-event pairs around every vs_* launch of every 4th step of the first region (events pre-created)
            ops.profile_reset(enable=True, pool=512 * (steps // 4 + 8))
        rk.barrier()
        t0 = time.perf_counter()
        if graphed is not None:
            for i in range(steps):
                loss = graphed.step()
        else:
            for i in range(steps):
                ops._PROF['on'] = events_on and rep == 0 and (i % 4 == 3 or steps < 8)
                loss = step()
        rk.barrier()
        regions.append(rk.max_over_ranks(time.perf_counter() - t0))
        ops._PROF['on'] = False
    if dump_dir is not None:
        dump_training_outputs(dump_dir, rk, net, opt, sync, loss)
    sampled = len([i for i in range(steps) if i % 4 == 3 or steps < 8])
    if graphed is not None and events_on:
        # per-kernel durations cannot be taken inside a graph replay (events are not recordable there): the same step is
        # run eagerly a few times afterwards with an event pair around every vs_* launch
        torch.cuda.synchronize()
        step()
        ops.profile_reset(enable=True, pool=1024 * (n_inst + 1))
        for i in range(n_inst):
            step()
        torch.cuda.synchronize()
        sampled = n_inst
    prof = ops.profile_collect() if events_on else {}
    err = int(rk.max_over_ranks(float(ops.rollout_exchange_error(dev))))
    if err:
        raise ExchangeTimeout('the rollout kernels reported an inter-workgroup exchange time-out (code %d): results are invalid '
                              '(VS_ROLLOUT_XCD_LOCAL=0 selects the placement-independent agent-scope exchange)' % err)
    final_loss = float(loss.item())
    n_all = sum(p.numel() for p in net.parameters())
    n_fused = sum(p.numel() for p in getattr(opt, '_fused', []))
    if n_fused:
        opt_text = ('Adam: %.1f M of %.1f M parameters updated in the epilogue of their weight-gradient GEMM (vs_gemm_adam), the rest by '
                    'one vs_adam_multi launch' % (n_fused / 1e6, n_all / 1e6))
    else:
        opt_text = 'Adam: vs_adam_multi (one HIP launch per 64 tensors%s)' % ('; one recording per all-reduce bucket' if sync is not None else '')
    out = {'cfg': cfg, 'ms': statistics.median(regions) / steps * 1e3, 'ms_all': [round(r / steps * 1e3, 4) for r in regions],
           'prof': prof, 'sampled': sampled, 'loss': final_loss, 'comm_bf16': comm_bf16, 'use_graph': use_graph,
           'scaler': None if scaler is None else scaler.describe(), 'optimizer': opt_text, 'precision': precision,
           'full_size': batch is None and not rk.ddp, 'graph': graph_stats}
    VF.fold_repeated_gradients(False)
    del graphed, net, opt, sync
    torch.cuda.empty_cache()
    return out


def run_eval(name, args, rk):
    """Inference throughput of workload `name`: frames emitted per second by eval-mode `get_forecast` over nt_cond + horizon frames."""
    from spatiotemporal_variable_separation_amd import functional as VF
    from spatiotemporal_variable_separation_amd.configs import BASELINE_CONFIGS
    from spatiotemporal_variable_separation_amd.data.synthetic import synthetic_batch
    from spatiotemporal_variable_separation_amd.networks.factory import build_sep_net
    cfg = dict(BASELINE_CONFIGS[name])
    if args.batch:
        cfg['batch'] = args.batch
    torch.manual_seed(1234)
    np.random.seed(1234)
    net = build_sep_net(cfg).to(rk.dev).eval()
    cond, _ = synthetic_batch(cfg['data'], cfg['batch'], cfg['nt_cond'], cfg['nt_pred'], device=rk.dev, seed=1234 + rk.rank)
    n = cfg['nt_cond'] + args.horizon
    VF.set_precision(args.precision)
    regions = []
    with torch.no_grad():
        for _ in range(max(1, args.warmup)):
            out = net.get_forecast(cond, n)[0]
        for _ in range(max(1, args.repeats)):
            rk.barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                out = net.get_forecast(cond, n)[0]
            rk.barrier()
            regions.append(rk.max_over_ranks(time.perf_counter() - t0))
    if args.dump_outputs and rk.rank == 0:
        os.makedirs(args.dump_outputs, exist_ok=True)
        f = _flat_sample([out])
        np.save(os.path.join(args.dump_outputs, 'forecast.npy'), f.reshape(tuple(out.shape)) if f.size == out.numel() else f)
    ms = statistics.median(regions) / args.steps * 1e3
    frames = rk.world * cfg['batch'] * n
    return {'metric': 'inference frames/sec (eval-mode get_forecast, frames emitted)', 'value': round(frames / (ms * 1e-3), 1), 'unit': 'frames/s',
            'n_gpus': rk.world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(ms, 4), 'higher_is_better': True, 'scaling': 'weak',
            'vs_baseline': None, 'dtype': args.precision, 'data': 'synthetic', 'ms_per_step_all': [round(r / args.steps * 1e3, 4) for r in regions],
            'config': {'workload': workload_text(name, cfg) + ', horizon %d (frames per call: %d)' % (args.horizon, n), 'global_batch': rk.world * cfg['batch'],
                       'parallelism': f'dp{rk.world} (independent replicas: inference has no exchange step)',
                       'mode': 'sep_net.eval(), torch.no_grad(), BatchNorm folded into the convolution weights, eager launches',
                       'output_checksum': round(float(out.float().mean().item()), 6)}}


def _latest_profile(workload, precision, kind):
    """Newest committed profiles/r<NN>_<workload>_<precision>_<kind>.json (static evidence collected by tools/collect_profiles.sh);
    returns (table, path, fresh): `fresh` = its `_source_sha` equals the sources this run executes."""
    import glob
    from spatiotemporal_variable_separation_amd.profiling import source_sha
    hits = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r[0-9][0-9]_%s_%s_%s.json' % (workload, precision, kind))))
    if not hits:
        return None, None, False
    try:
        tab = json.load(open(hits[-1]))
    except (OSError, ValueError):
        return None, None, False
    return tab, 'profiles/' + os.path.basename(hits[-1]), tab.get('_source_sha') == source_sha()


def live_replay_table(workload, precision, steps, warmup, timeout_s=240):
    """Per-group kernel time of the REPLAYED step, measured in this run: the same command as a child process under
    `rocprofv3 --kernel-trace --stats` (VARSEP_BENCH_NO_EVENTS=1: no instrumented eager steps, so every launch in the table but the
    recording's warm-up is a graph replay), kernel statistics read back through profiling.replay_table.  Called BEFORE this process touches
    the GPU (the child owns the device meanwhile).  Returns {'groups', 'steps', 'unassigned_us_per_step'} or None (no rocprofv3, time-out,
    failure: the caller falls back)."""
    import csv
    import glob
    import shutil
    import tempfile
    from spatiotemporal_variable_separation_amd.profiling import replay_table
    tool = shutil.which('rocprofv3') or ('/opt/rocm/bin/rocprofv3' if os.path.exists('/opt/rocm/bin/rocprofv3') else None)
    if tool is None:
        return None
    tmp = tempfile.mkdtemp(prefix='varsep_prof_', dir='/tmp')
    env = dict(os.environ, VARSEP_BENCH_NO_EVENTS='1', VARSEP_BENCH_LIVE_PROFILE='0', TMPDIR='/tmp')
    cmd = [tool, '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'p', '--', sys.executable, os.path.abspath(__file__),
           '--config', workload, '--precision', precision, '--steps', str(steps), '--warmup', str(warmup), '--repeats', '2',
           '--no_cpu_baseline', '--extra_configs', 'none']
    try:
        t0 = time.time()
        # a session of its own: on a time-out the WHOLE process group goes (rocprofv3 is a launcher; killing it alone would leave the
        # benchmark grandchild running on the GPU while this process starts its timed regions)
        proc = subprocess.Popen(cmd, env=env, cwd='/tmp', stdout=subprocess.PIPE, stderr=subprocess.PIPE, start_new_session=True)
        try:
            out, err = proc.communicate(timeout=timeout_s)
        except subprocess.TimeoutExpired:
            import signal
            try:
                os.killpg(proc.pid, signal.SIGKILL)
            except OSError:
                pass
            proc.communicate()
            sys.stderr.write('bench.py: live rocprofv3 pass of %s timed out after %d s (process group killed)\n' % (workload, timeout_s))
            return None
        hits = glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True)
        if proc.returncode != 0 or not hits:
            sys.stderr.write('bench.py: live rocprofv3 pass of %s failed (rc %s): %s\n' % (workload, proc.returncode, err.decode(errors='replace')[-400:]))
            return None
        rows = list(csv.DictReader(open(hits[0])))
        nsteps, table, rest = replay_table(rows)
        child = None
        for ln in out.decode(errors='replace').splitlines():
            if ln.startswith('{'):
                child = json.loads(ln)
        return {'groups': table, 'steps': nsteps, 'unassigned_us_per_step': rest, 'seconds': round(time.time() - t0, 1),
                'profiled_ms_per_step': None if child is None else child.get('ms_per_step')}
    except (OSError, ValueError) as e:
        sys.stderr.write('bench.py: live rocprofv3 pass of %s: %s\n' % (workload, e))
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def rooflines(res, workload, precision, top=6, live=None):
    """Roofline position of every kernel GROUP (spatiotemporal_variable_separation_amd/profiling.py), largest time per step first.

    Algorithmic FLOPs / bytes per step: the live accounting of this run (ops.profile_collect over the instrumented steps).  Duration of a
    group, in order of preference: (1) `replay-live`: kernel statistics of this run's own rocprofv3 child pass over the replayed step
    (live_replay_table); (2) `replay-committed`: the committed table under profiles/ when its source hash still matches; (3) `eager`: HIP
    events around every launch of the instrumented eager steps (always computed, printed beside the others in bench_detail.json)."""
    from spatiotemporal_variable_separation_amd.profiling import bound_of, group_of_family
    prof, ms, sampled = res['prof'], res['ms'], res['sampled']
    if not prof:
        return None, []
    replay, replay_src, timing, stale = (None, None, 'eager', False)
    traffic, traffic_src, traffic_fresh = (None, None, False)
    if res.get('full_size', True):
        traffic, traffic_src, traffic_fresh = _latest_profile(workload, precision, 'traffic')
        if live is not None:
            replay, replay_src, timing = live, 'rocprofv3 --kernel-trace --stats child pass of this run (%d steps)' % live['steps'], 'replay-live'
        else:
            tab, src, fresh = _latest_profile(workload, precision, 'replay')
            if tab is not None and fresh:
                replay, replay_src, timing = tab, src, 'replay-committed'
            elif tab is not None:
                stale = True
    groups = {}
    for name, rec in prof.items():
        g = group_of_family(name) or name
        e = groups.setdefault(g, {'ms': 0.0, 'n': 0, 'flops': 0.0, 'bytes': 0.0, 'families': []})
        for k in ('ms', 'n', 'flops', 'bytes'):
            e[k] += rec[k]
        e['families'].append(name)
    peak_mfma = 157.3 if precision == 'fp32' else 2500.0

    def roof_of(g, e):
        bound = bound_of(g) if e['flops'] > 0 or bound_of(g) == 'hbm' else 'hbm'
        work = (e['flops'] if bound == 'mfma' else e['bytes']) / sampled              # algorithmic FLOPs or bytes per step
        peak, unit, scale = (peak_mfma, 'TFLOP/s', 1e12) if bound == 'mfma' else (8000.0, 'GB/s', 1e9)
        eager_us = e['ms'] * 1e3 / sampled
        eager = {'us_per_step': round(eager_us, 1), 'avg_launch_us': round(e['ms'] * 1e3 / e['n'], 2),
                 'achieved': round(work / (eager_us * 1e-6) / scale, 2), 'frac': round(work / (eager_us * 1e-6) / scale / peak, 4)}
        out = {'kernel': g, 'families': sorted(e['families']), 'bound': bound, 'peak': peak, 'unit': unit,
               'algorithmic_per_step': round(work), 'algorithmic_bytes_per_step': round(e['bytes'] / sampled)}
        rp = (replay or {}).get('groups', {}).get(g)
        if rp:
            us = rp['us_per_step']
            # the share of the step is taken inside ONE run: the profiled child's kernel time over the profiled child's own step time (kernel
            # times of the profiled pass over the un-profiled parent's step mixed two runs: advisor finding, round 4); sums above 1 mean
            # overlapping streams
            step_ms = (replay.get('profiled_ms_per_step') or ms) if timing == 'replay-live' else ms
            out.update({'achieved': round(work / (us * 1e-6) / scale, 2), 'frac': round(work / (us * 1e-6) / scale / peak, 4),
                        'launches_per_step': round(rp['launches_per_step'], 2), 'avg_launch_us': round(rp['avg_launch_us'], 3), 'us_per_step': round(us, 1),
                        'share_of_step': round(us * 1e-3 / step_ms, 3), 'timing': timing, 'source': replay_src, 'eager_events': eager})
        else:
            out.update({'achieved': eager['achieved'], 'frac': eager['frac'], 'launches_per_step': round(e['n'] / sampled, 2),
                        'avg_launch_us': eager['avg_launch_us'], 'us_per_step': eager['us_per_step'], 'share_of_step': round(eager_us * 1e-3 / ms, 3),
                        'timing': 'eager', 'source': 'live HIP events around every launch of %d eager steps' % sampled})
            if stale:
                out['stale'] = True           # a committed replay table exists but was collected on other kernel sources: not used
        tr = (traffic or {}).get('groups', {}).get(g)
        out['traffic'] = None
        if tr:
            out['traffic'] = round(tr['bytes_per_launch'])
            out['traffic_per_step'] = round(tr['bytes_per_step'])
            out['traffic_source'] = traffic_src
            if not traffic_fresh:
                out['traffic_stale'] = True   # PMC passes of an earlier source state (profiles/ names the round)
        if 'rollout' in g:
            out['note'] = ('sequential recurrence: (n-1)*n_blocks*3 dependent 16-row GEMMs per slab, bound by the inter-workgroup exchange '
                           'latency, not by MFMA rate (SURVEY.md H3)')
        return out
    roofs = [roof_of(g, e) for g, e in groups.items()]
    roofs.sort(key=lambda r: -r['us_per_step'])
    # BOTH roofs of the dominant group and of the whole step: which one is nearer.  Bytes: the PMC traffic table when
    # one exists for these sources, the algorithmic bytes otherwise (`bytes_from`); step-level sums run over every group.
    top_g = roofs[0]
    grp_bytes = top_g.get('traffic_per_step') if (top_g.get('traffic_per_step') and not top_g.get('traffic_stale')) else top_g['algorithmic_bytes_per_step']
    tot_flops = sum(e['flops'] for e in groups.values()) / sampled
    tot_alg_bytes = sum(e['bytes'] for e in groups.values()) / sampled
    tot_traffic = sum(t_['bytes_per_step'] for t_ in (traffic or {}).get('groups', {}).values()) if (traffic and traffic_fresh) else None
    step_s = ms * 1e-3
    both = {'group_mfma': round(sum(e['flops'] for g_, e in groups.items() if g_ == top_g['kernel']) / sampled / (top_g['us_per_step'] * 1e-6) / 1e12 / peak_mfma, 4),
            'group_hbm': round(grp_bytes / (top_g['us_per_step'] * 1e-6) / 1e9 / 8000.0, 4),
            'step_mfma': round(tot_flops / step_s / 1e12 / peak_mfma, 4),
            'step_hbm': round((tot_traffic if tot_traffic else tot_alg_bytes) / step_s / 1e9 / 8000.0, 4),
            'bytes_from': 'pmc' if tot_traffic else 'algorithmic'}
    both['nearer_roof'] = 'hbm' if both['step_hbm'] > both['step_mfma'] else 'mfma'
    top_g['both_bounds'] = both
    if replay:
        # kernel launches of one replayed step, all groups (the recording's kernel nodes): into the dominant group's
        # object so that the line and bench_detail.json carry it
        roofs[0]['kernel_launches_per_step'] = round(sum(g_['launches_per_step'] for g_ in replay.get('groups', {}).values()), 1)
    return roofs[0], roofs[1:top]


_ROOF_KEYS = ('kernel', 'bound', 'peak', 'unit', 'achieved', 'frac', 'us_per_step', 'launches_per_step', 'kernel_launches_per_step', 'avg_launch_us', 'share_of_step',
              'traffic', 'traffic_per_step', 'algorithmic_bytes_per_step', 'algorithmic_per_step', 'timing', 'source', 'stale', 'traffic_stale', 'both_bounds')


def compact_line(full, limit=4000):
    """The ONE stdout line (< 4 KB: the driver reads an 8 KB tail) from the full result: headline fields, the dominant group's roofline,
    cpu_baseline and one short entry per further workload.  Everything dropped here is in bench_detail.json."""
    out = {k: full[k] for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                                'vs_baseline', 'dtype', 'data') if k in full}
    cfg = full.get('config', {})
    out['config'] = {k: cfg[k] for k in ('workload', 'global_batch', 'parallelism', 'grad_allreduce', 'launch', 'final_loss') if k in cfg}
    if 'roofline' in full:                   # (--full)
        rf = full['roofline']
        out['roofline'] = None if rf is None else {k: rf[k] for k in _ROOF_KEYS if k in rf}
    if full.get('graph'):
        out['graph'] = full['graph']
    cb = full.get('cpu_baseline')
    if cb is not None:
        out['cpu_baseline'] = {k: cb[k] for k in ('value', 'unit', 'cores', 'ms_per_step', 'kind', 'sample', 'by_threads_ms_per_step') if k in cb}
    if full.get('configs'):
        out['configs'] = {}
        for name, c in full['configs'].items():
            if 'error' in c:
                out['configs'][name] = {'error': c['error'][:120]}
                continue
            r = c.get('roofline') or {}
            out['configs'][name] = {'ms_per_step': c['ms_per_step'], 'value': c['value'], 'dtype': c['dtype'], 'n_gpus': c['n_gpus'],
                                    'roofline': {k: r[k] for k in ('kernel', 'bound', 'frac', 'achieved', 'unit', 'timing') if k in r}}
    out['detail'] = 'bench_detail.json'
    line = json.dumps(out)
    # belt and braces: shed optional fields until the line fits
    for drop in (('cpu_baseline', 'sample'), ('cpu_baseline', 'by_threads_ms_per_step'), ('roofline', 'source'), ('config', 'launch'), ('configs', None)):
        if len(line) <= limit:
            break
        if drop[1] is None:
            out.pop(drop[0], None)
        elif isinstance(out.get(drop[0]), dict):
            out[drop[0]].pop(drop[1], None)
        line = json.dumps(out)
    assert len(line) <= limit, len(line)
    return line


def allreduce_text(rk, res):
    if not rk.ddp:
        return 'none (1 rank)'
    return '%s buckets over %s' % ('bf16' if res['comm_bf16'] else 'fp32', 'RCCL' if rk.backend == 'nccl' else 'gloo (ranks share one GPU: test mode)')


def workload_text(name, cfg):
    return (f'{name}: {cfg["architecture"]} enc/dec, batch {cfg["batch"]}/GPU, nt_cond {cfg["nt_cond"]}, '
            f'nt_pred {cfg["nt_pred"]}, offset {cfg["offset"]}')


def main():
    args = parse()
    if args.graph_stats:
        os.environ['VARSEP_GRAPH_STATS'] = '1'
    if args.gpus > 1 and 'RANK' not in os.environ:
        spawn_ranks(args)                    # does not return
    # stdout carries exactly ONE line (the result JSON): libraries that print banners to the C-level stdout (RCCL prints its
    # version block there at communicator creation) are diverted to stderr for the whole run
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get('WORLD_SIZE', 1))
    force_dist = os.environ.get('VARSEP_BENCH_FORCE_DIST') == '1'
    extra = args.extra_configs
    if extra is None:
        if args.full and args.config == 'waveeq' and args.batch is None and args.precision == 'bf16':
            extra = EXTRA_DEFAULT if (world == 1 and not force_dist) else EXTRA_DEFAULT_DIST
        else:
            extra = 'none'
    extra_names = [e for e in extra.split(',') if e and e != 'none']

    # per-kernel clock of the replayed step, measured in this run: child passes under rocprofv3 BEFORE this process touches the GPU
    live = {}
    mode = os.environ.get('VARSEP_BENCH_LIVE_PROFILE', 'all')
    if (args.full and mode != '0' and world == 1 and not force_dist and not args.eval_mode and not args.no_graph and args.batch is None
            and os.environ.get('VARSEP_BENCH_NO_EVENTS') is None):
        t_start = time.time()
        todo = [(args.config, args.precision, args.steps, args.warmup)]
        if mode == 'all':
            for name in extra_names:
                wname, prec = split_workload(name, args.precision)
                st, wu = EXTRA_STEPS.get(name, (5, 2))
                todo.append((wname, prec, st, wu))
        for wname, prec, st, wu in todo:
            if time.time() - t_start > 200:          # the default run has to finish within minutes: later workloads fall back
                break
            tab = live_replay_table(wname, prec, st, wu)
            if tab is not None:
                live[(wname, prec)] = tab
                sys.stderr.write('bench.py: live replay table of %s/%s: %d steps, %.1f s\n' % (wname, prec, tab['steps'], tab['seconds']))

    rk = Ranks(args)
    if args.eval_mode:
        line = run_eval(args.config, args, rk)
        if rk.rank == 0:
            os.write(result_fd, (json.dumps(line) + '\n').encode())
        rk.close()
        return
    res = run_workload(args.config, args, rk, args.steps, args.warmup, args.repeats, batch=args.batch, dump_dir=args.dump_outputs)

    # further workloads under "configs".  Every rank runs them (they contain the same barriers / all-reduces); rank 0 reports.
    configs = None
    if extra_names:
        configs = {}
        for name in extra_names:
            st, wu = EXTRA_STEPS.get(name, (5, 2))
            wname, prec = split_workload(name, args.precision)
            err = None
            try:
                r = run_workload(wname, args, rk, st, wu, 3, precision=prec)
            except Exception as e:          # one workload failing must not take the headline line down; it is reported
                err = '%s: %s' % (type(e).__name__, str(e)[:300])
            if rk.ddp:
                # every rank reaches this point (a failure that is deterministic in the code path hits all of them alike); the workload
                # counts only if it succeeded everywhere
                bad = rk.max_over_ranks(1.0 if err else 0.0)
                if bad and not err:
                    err = 'failed on another rank'
            if err:
                configs[name] = {'error': err}
                continue
            c = r['cfg']
            rf, oth = rooflines(r, wname, prec, top=4, live=live.get((wname, prec)))
            configs[name] = {'workload': workload_text(wname, c), 'ms_per_step': round(r['ms'], 4), 'n_gpus': rk.world,
                             'value': round(rk.world * c['batch'] * c['nt_pred'] / (r['ms'] * 1e-3), 1), 'unit': 'frames/s',
                             'steps': st, 'warmup': wu, 'ms_per_step_all': r['ms_all'], 'dtype': prec,
                             'grad_allreduce': allreduce_text(rk, r), 'optimizer': r['optimizer'], 'final_loss': round(r['loss'], 5), 'graph': r.get('graph'),
                             'roofline': rf, 'roofline_others': oth}
            if r['scaler']:
                configs[name]['loss_scaling'] = r['scaler']
    if rk.rank != 0:
        rk.close()
        return
    cfg, ms = res['cfg'], res['ms']
    frames = rk.world * cfg['batch'] * cfg['nt_pred']
    launch = 'hipGraph replay' if res['use_graph'] else 'eager'
    out = {
        'metric': 'training frames/sec (seq x nt_pred)', 'value': round(frames / (ms * 1e-3), 1), 'unit': 'frames/s',
        'n_gpus': rk.world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(ms, 4),
        'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': args.precision, 'data': 'synthetic',
        'repeats': len(res['ms_all']), 'ms_per_step_all': res['ms_all'],
        'config': {'workload': workload_text(args.config, cfg),
                   'global_batch': rk.world * cfg['batch'], 'parallelism': f'dp{rk.world}',
                   'grad_allreduce': allreduce_text(rk, res), 'optimizer': res['optimizer'], 'launch': launch,
                   'timing': 'median of %d regions of %d steps' % (len(res['ms_all']), args.steps),
                   'final_loss': round(res['loss'], 5)},
        # nodes / kernel nodes / dependency edges / roots of the recorded step (train.GraphedStep.graph_stats): what one replay costs the host
        'graph': res.get('graph'),
    }
    if args.full:
        out['roofline'], out['roofline_others'] = rooflines(res, args.config, args.precision, live=live.get((args.config, args.precision)))
    if out.get('graph') is None and args.full:
        tab, src, fresh = _latest_profile(args.config, args.precision, 'graph')
        if tab is not None and fresh:
            out['graph'] = dict({k: tab[k] for k in ('nodes', 'kernel_nodes', 'edges', 'roots') if k in tab}, source=src)
    elif args.graph_stats:
        try:
            from spatiotemporal_variable_separation_amd.profiling import source_sha as _sha
            os.makedirs(os.path.join(ROOT, 'gpurun_out'), exist_ok=True)
            with open(os.path.join(ROOT, 'gpurun_out', 'graph_stats_%s_%s.json' % (args.config, args.precision)), 'w') as f:
                json.dump(dict(out['graph'], _source_sha=_sha(), _source='python bench.py --config %s --precision %s --graph_stats' % (args.config, args.precision)), f)
        except OSError:
            pass
    if res['scaler']:
        out['config']['loss_scaling'] = res['scaler']
    if configs is not None:
        out['configs'] = configs
    if live:
        out['live_profile'] = {'%s/%s' % k: {kk: v[kk] for kk in ('steps', 'seconds', 'profiled_ms_per_step', 'unassigned_us_per_step')}
                               for k, v in live.items()}
    if args.full and rk.world == 1 and not args.no_cpu_baseline:
        steps = args.cpu_steps or (5 if args.config in ('waveeq', 'mnist_b16') else 2)
        out['cpu_baseline'] = cpu_baseline(cfg, steps)
    from spatiotemporal_variable_separation_amd.profiling import source_sha
    out['source_sha'] = source_sha()
    detail = json.dumps(out, indent=1)
    try:
        with open(os.path.join(ROOT, 'bench_detail.json'), 'w') as f:
            f.write(detail + '\n')
    except OSError:
        pass
    sys.stderr.write(detail + '\n')
    sys.stderr.flush()
    os.write(result_fd, (compact_line(out) + '\n').encode())
    rk.close()


if __name__ == '__main__':
    main()

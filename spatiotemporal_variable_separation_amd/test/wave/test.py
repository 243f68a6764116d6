"""WaveEq evaluation (reference: test/wave/test.py:30-98, same flags):

    python -m spatiotemporal_variable_separation_amd.test.wave.test --xp_dir X --data_dir D --device 0

Forecasts 40 frames of every test window (`wave`: full frames, `wave_partial`: the pixel subset) from the HBM-resident WaveEq sets and
prints the mean MSE over the horizon.  `--data_dir simulated` evaluates on the test half of the set simulated on the device (what main.py
trains on under the same value).  There is no CPU mode: --device is required.
"""
from ...data.wave_eq import WaveEq, WaveEqPartial
from ..utils import add_precision_flag, base_parser, forecast_metrics, horizon_mse_main


def load_dataset(args, train=False):
    if args.data_dir == 'simulated':                                # the set main.py trains on under the same value: simulated in HBM, no files
        if args.data == 'wave':
            return WaveEq.simulated(args.nt_cond, args.nt_cond + args.nt_pred, train, args.downsample, device=args.device)
        return WaveEqPartial.simulated(args.nt_cond, args.nt_cond + args.nt_pred, train, args.downsample, args.n_wave_points, device=args.device)
    if args.data == 'wave':
        return WaveEq(args.data_dir, args.nt_cond, args.nt_cond + args.nt_pred, train, args.downsample, device=args.device)
    return WaveEqPartial(args.data_dir, args.nt_cond, args.nt_cond + args.nt_pred, train, args.downsample, args.n_wave_points,
                         device=args.device)


def compute_mse(args, batch_size, test_set, sep_net):
    """Per-frame MSE of every test window: [B, T] per batch for `wave`, [B, T, 1] for `wave_partial` (test/wave/test.py:38-58)."""
    if args.data == 'wave':
        return forecast_metrics(args, batch_size, test_set, sep_net, lambda f, t: [(f - t).pow(2).mean(dim=-1).mean(dim=-1).mean(dim=-1)])[0]
    return forecast_metrics(args, batch_size, test_set, sep_net, lambda f, t: [(f - t).pow(2).mean(dim=-1)])[0]


def main(args):
    return horizon_mse_main(args, 40, load_dataset, compute_mse)


def build_parser():
    p = base_parser('PDE-Driven Spatiotemporal Disentanglement (Moving MNIST testing)', batch_size=256, nt_pred=False)
    return add_precision_flag(p)


if __name__ == '__main__':
    main(build_parser().parse_args())

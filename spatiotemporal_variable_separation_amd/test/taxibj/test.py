"""TaxiBJ evaluation (reference: test/taxibj/test.py:37-93, same flags plus --batch_size and --precision):

    python -m spatiotemporal_variable_separation_amd.test.taxibj.test --xp_dir X --data_dir D --device 0

Forecasts 4 frames of every window of the test half (the last 48 * 7 * 4 windows) from the HBM-resident TaxiBJ set and prints the mean MSE
over the horizon.  The reference feeds the windows one by one (batch size 1); the networks run in eval mode, where BatchNorm uses its
running statistics and every window is computed independently of its batch, so batching gives the same per-window values.  There is no
CPU mode: --device is required.
"""
from ...data.taxibj import TaxiBJ
from ..utils import add_precision_flag, base_parser, forecast_metrics, horizon_mse_main


def load_dataset(args):
    return TaxiBJ.make_datasets(args.data_dir, len_closeness=args.nt_cond + args.nt_pred, nt_cond=args.nt_cond, device=args.device)[1]


def compute_mse(args, batch_size, test_set, sep_net):
    """Per-frame MSE of every test window, [B, T] per batch (test/taxibj/test.py:41-56), computed on the device."""
    return forecast_metrics(args, batch_size, test_set, sep_net, lambda f, t: [(f - t).pow(2).mean(dim=-1).mean(dim=-1).mean(dim=-1)])[0]


def main(args):
    return horizon_mse_main(args, 4, load_dataset, compute_mse)


def build_parser():
    p = base_parser('PDE-Driven Spatiotemporal Disentanglement (Moving MNIST testing)', batch_size=256, nt_pred=False)
    return add_precision_flag(p)


if __name__ == '__main__':
    main(build_parser().parse_args())

"""SST evaluation (reference: test/sst/test.py:29-117, same flags plus --batch_size and --precision):

    python -m spatiotemporal_variable_separation_amd.test.sst.test --xp_dir X --data_dir D --device 0

Forecasts 10 days of every window of the test half (the last fifth of the days) of zones 17-20 from the HBM-resident SST set and prints MSE
and SSIM at t+10 and t+6 in original units.  The reference feeds the windows one by one; the networks run in eval mode, where BatchNorm uses
its running statistics and every window is computed independently of its batch, so batching gives the same per-window values.

The script's numbers have a property its text does not show: the per-day constants leave the dataset as [10, 1, 1] arrays and are
multiplied into [1, 10, 1, 64, 64] forecasts, so broadcasting turns the channel axis into a second day axis.  `mse` [N, 10] is a mean over
that axis as well, `ssim` is [N, 10, 10] -- frame t under the constants of day c -- and the printed SSIM is the mean over all pairs; the
zone's min / max of the rescale are those of the z-scored data while the frames they rescale are back in original units.  These are the
paper's numbers, so all of it is reproduced (utils/metrics.py: sst_metrics, one `vs_sst_frame_metrics` launch per batch).  There is no CPU
mode: --device is required.
"""
import numpy as np

from ...data.sst import SST
from ...utils.metrics import sst_metrics
from ..utils import add_precision_flag, base_parser, forecast_metrics, load_model, load_xp_config, setup_device


def load_dataset(args, train=False, zones=range(17, 21)):
    return SST(args.data_dir, args.nt_cond, args.nt_pred, train, zones=zones, eval=True, device=args.device)


def compute_mse_ssim(args, batch_size, test_set, sep_net):
    """Per-window MSE [B, T] and SSIM [B, T, T] per batch (test/sst/test.py:41-76), computed on the device."""
    return forecast_metrics(args, batch_size, test_set, sep_net,
                            lambda f, t, day0, zone: sst_metrics(f, t, test_set.consts, day0, zone, test_set.zone_range))


def main(args):
    device = setup_device(args)
    xp_config = load_xp_config(args, device, 10)         # the reference evaluates at t+10 whatever the training horizon
    args.nt_pred = 10

    test_set = load_dataset(xp_config, train=False)
    sep_net = load_model(xp_config, args.epoch)

    all_mse, all_ssim = compute_mse_ssim(xp_config, args.batch_size, test_set, sep_net)
    mse_array = np.concatenate(all_mse, axis=0)
    ssim_array = np.concatenate(all_ssim, axis=0)
    print(f'MSE at t+10: {np.mean(mse_array.mean(axis=0)[:10])}')
    print(f'MSE at t+6: {np.mean(mse_array.mean(axis=0)[:6])}')
    print(f'SSIM at t+10: {np.mean(ssim_array.mean(axis=0)[:10])}')
    print(f'SSIM at t+6: {np.mean(ssim_array.mean(axis=0)[:6])}')
    return mse_array, ssim_array


def build_parser():
    p = base_parser('PDE-Driven Spatiotemporal Disentanglement (Moving MNIST testing)', batch_size=256, nt_pred=False)
    return add_precision_flag(p)


if __name__ == '__main__':
    main(build_parser().parse_args())

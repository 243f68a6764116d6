"""TaxiBJ evaluation (reference: test/taxibj/test.py:37-93, same flags plus --batch_size and --precision):

    python -m spatiotemporal_variable_separation_amd.test.taxibj.test --xp_dir X --data_dir D --device 0

Forecasts 4 frames of every window of the test half (the last 48 * 7 * 4 windows) from the HBM-resident TaxiBJ set and prints the mean MSE
over the horizon.  The reference feeds the windows one by one (batch size 1); the networks run in eval mode, where BatchNorm uses its
running statistics and every window is computed independently of its batch, so batching gives the same per-window values.  There is no
CPU mode: --device is required.
"""
import os

import numpy as np
import torch

from ...data.taxibj import TaxiBJ
from ...data.wave_eq import DeviceBatchLoader
from ...utils.helper import load_json
from ..utils import add_precision_flag, base_parser, load_model, setup_device


def load_dataset(args):
    return TaxiBJ.make_datasets(args.data_dir, len_closeness=args.nt_cond + args.nt_pred, nt_cond=args.nt_cond, device=args.device)[1]


def compute_mse(args, batch_size, test_set, sep_net):
    """Per-frame MSE of every test window, [B, T] per batch (test/taxibj/test.py:41-56), computed on the device."""
    all_mse = []
    loader = DeviceBatchLoader(test_set, batch_size, shuffle=False)
    torch.set_grad_enabled(False)
    for cond, target in loader:
        if args.offset:
            forecasts = sep_net.get_forecast(cond, target.size(1) + args.nt_cond)[0]
            forecasts = forecasts[:, args.nt_cond:]
        else:
            forecasts = sep_net.get_forecast(cond, target.size(1))[0]

        forecasts = forecasts.float().reshape(target.shape)
        mse = (forecasts - target).pow(2).mean(dim=-1).mean(dim=-1).mean(dim=-1)

        all_mse.append(mse.cpu().numpy())

    return all_mse


def main(args):
    device = setup_device(args)
    xp_config = load_json(os.path.join(args.xp_dir, 'params.json'))
    xp_config.device = device
    xp_config.data_dir = args.data_dir
    xp_config.xp_dir = args.xp_dir
    xp_config.nt_pred = 4           # the reference evaluates at t+4 whatever the training horizon
    args.nt_pred = 4

    test_set = load_dataset(xp_config)
    sep_net = load_model(xp_config, args.epoch)

    all_mse = compute_mse(xp_config, args.batch_size, test_set, sep_net)
    mse_array = np.concatenate(all_mse, axis=0)
    print(f'MSE at t+4: {np.mean(mse_array.mean(axis=0)[:4])}')
    return mse_array


def build_parser():
    p = base_parser('PDE-Driven Spatiotemporal Disentanglement (Moving MNIST testing)', batch_size=256, nt_pred=False)
    add_precision_flag(p)
    return p


if __name__ == '__main__':
    main(build_parser().parse_args())

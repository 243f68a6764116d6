"""WaveEq evaluation (reference: test/wave/test.py:30-98, same flags):

    python -m spatiotemporal_variable_separation_amd.test.wave.test --xp_dir X --data_dir D --device 0

Forecasts 40 frames of every test window (`wave`: full frames, `wave_partial`: the pixel subset) from the HBM-resident WaveEq sets and
prints the mean MSE over the horizon.  There is no CPU mode: --device is required.
"""
import os

import numpy as np
import torch

from ...data.wave_eq import DeviceBatchLoader, WaveEq, WaveEqPartial
from ...utils.helper import load_json
from ..utils import add_precision_flag, base_parser, load_model, setup_device


def load_dataset(args, train=False):
    if args.data == 'wave':
        return WaveEq(args.data_dir, args.nt_cond, args.nt_cond + args.nt_pred, train, args.downsample, device=args.device)
    return WaveEqPartial(args.data_dir, args.nt_cond, args.nt_cond + args.nt_pred, train, args.downsample, args.n_wave_points,
                         device=args.device)


def compute_mse(args, batch_size, test_set, sep_net):
    """Per-frame MSE of every test window: [B, T] per batch for `wave`, [B, T, 1] for `wave_partial` (test/wave/test.py:38-58)."""
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

        if args.data == 'wave':
            mse = (forecasts - target).pow(2).mean(dim=-1).mean(dim=-1).mean(dim=-1)
        else:
            mse = (forecasts - target).pow(2).mean(dim=-1)

        all_mse.append(mse.cpu().numpy())

    return all_mse


def main(args):
    device = setup_device(args)
    xp_config = load_json(os.path.join(args.xp_dir, 'params.json'))
    xp_config.device = device
    xp_config.data_dir = args.data_dir
    xp_config.xp_dir = args.xp_dir
    xp_config.nt_pred = 40          # the reference evaluates at t+40 whatever the training horizon
    args.nt_pred = 40

    test_set = load_dataset(xp_config, train=False)
    sep_net = load_model(xp_config, args.epoch)

    all_mse = compute_mse(xp_config, args.batch_size, test_set, sep_net)
    mse_array = np.concatenate(all_mse, axis=0)
    print(f'MSE at t+40: {np.mean(mse_array.mean(axis=0)[:40])}')
    return mse_array


def build_parser():
    p = base_parser('PDE-Driven Spatiotemporal Disentanglement (Moving MNIST testing)', batch_size=256, nt_pred=False)
    add_precision_flag(p)
    return p


if __name__ == '__main__':
    main(build_parser().parse_args())

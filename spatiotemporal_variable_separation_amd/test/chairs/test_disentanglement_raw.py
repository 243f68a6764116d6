"""The 3D Warehouse Chairs content-swap evaluation of test_disentanglement.py on the ORIGINAL renders, with no prepared files:

    python -m spatiotemporal_variable_separation_amd.test.chairs.test_disentanglement_raw --xp_dir X --data_dir D --nt_pred 10 --device 0

Same flags, seeds, batches, metrics and output files as test_disentanglement.py; --data_dir holds the raw `renders/<name>.png` (600 x 600 in
the original set, exactly 62 per object), which are cropped and resized on the device straight into HBM (`Chairs.from_raw`,
csrc/vs_resample.hip) as preprocessing/chairs/gen_chairs.py would prepare them.  On renders that gen_chairs has also prepared, both
scripts hold the same bytes and write the same results.  Additive `--chairs_box` (options.py) for renders of another size.  This is
what `--chairs_raw` is to main.py; it is a module of its own so that test_disentanglement.py keeps the reference's surface untouched.
"""
import torch

from ...data.chairs import Chairs
from ...options import add_chairs_box_flag
from ..utils import load_model, load_xp_config, run_content_swap, seed_all, setup_device
from . import test_disentanglement as prepared


def main(args):
    device = setup_device(args)
    seed_all(args.test_seed)
    xp_config = load_xp_config(args, device, args.nt_pred)
    xp_config.n_object = 1           # as test_disentanglement.py

    print('Loading data...')
    seq_len = xp_config.nt_cond + args.nt_pred
    test_dataset = Chairs.from_raw(False, args.data_dir, xp_config.nt_cond, seq_len=seq_len, box=args.chairs_box, device=device)
    swap_dataset = prepared.SwapDataset.from_raw(False, args.data_dir, xp_config.nt_cond, seq_len=seq_len, box=args.chairs_box, device=device)

    print('Loading model...')
    sep_net = load_model(xp_config, args.epoch)

    print('Generating samples...')
    torch.set_grad_enabled(False)
    return run_content_swap(args.xp_dir, sep_net, xp_config.nt_cond, seq_len, prepared.swap_batches(test_dataset, swap_dataset, args.batch_size))


def build_parser():
    p = prepared.build_parser()
    add_chairs_box_flag(p)
    return p


if __name__ == '__main__':
    main(build_parser().parse_args())

"""Moving-MNIST evaluation (reference: test/mnist/test.py:50-188, same flags and output files):

    python -m spatiotemporal_variable_separation_amd.test.mnist.test --xp_dir X --data_dir D --nt_pred 95 --device 0

Forecasts the test set (MSE / PSNR / SSIM per sample, printed as the reference's `Results:` block) and a content swap: the S code of
each test video drives a forecast from a freshly generated training video.  The test set lives in HBM, the swap videos are rendered by
the device generator from the global NumPy stream in the reference's order, the metrics run on the device (vs_frame_metrics) and every
saved array is converted to uint8 on the device (vs_frames_to_u8_nhwc).  There is no CPU mode: --device is required.
`--data_dir generated:D` needs only the raw MNIST idx files under D: the test set that preprocessing/mnist/make_test_set.py would write
with its defaults is generated straight into HBM (`MovingMNIST.generated`), no .npz is read or written.
`--mnist_stochastic` evaluates a model trained with `main --mnist_stochastic`: the test set is the stochastic one (smmnist_test_*.npz, or
generated with the prefix) and the swap videos come from the stochastic sampler; test_disentanglement_stochastic.py is the content swap on it.
Who compresses the six frame files: the environment variable VARSEP_NPZ_COMPRESS=host|device (utils/savez.py), read once at the start of
`main`.  `host` (the default) copies every batch's uint8 frames to the host and writes with np.savez_compressed, as before; `device` keeps
them in HBM, compresses them there and downloads only the compressed bytes.  Names, keys, dtypes, shapes and the arrays np.load gives are
the same; measurements and the sizes of the device-written files: profiles/eval_npz_timing.md.
Who decompresses the test-set file D/[s]mmnist_test_*.npz: VARSEP_NPZ_LOAD=host|device (utils/loadz.py), read once at the same place.
`host` (the default) is np.load and the host conversion, as before; `device` uploads the compressed bytes and inflates them in HBM.
With `device`, VARSEP_NPZ_FOREIGN=host|device (read at that same place) says who inflates a file that is not cut at sync markers, as
np.savez_compressed writes it: the host (the default) or the block-parallel reader of csrc/vs_inflate_blocks.hip.  With both `device`,
VARSEP_NPZ_FINDER=dynamic|all (read there too) says whether that reader starts at dynamic block headers alone (the default) or at stored
ones as well.
"""
import os

import torch

from ...data.moving_mnist import MovingMNIST
from ...utils import loadz, savez
from ...utils.metrics import frame_metrics
from ..utils import U8Frames, add_precision_flag, base_parser, load_model, load_xp_config, print_results, seed_all, setup_device


GENERATED = 'generated:'         # --data_dir generated:D: the idx files are under D and the test set is generated in HBM, no .npz is read


def split_data_dir(data_dir):
    """(directory of the MNIST files, whether the test set is generated on the device instead of read from its file)."""
    return (data_dir[len(GENERATED):], True) if data_dir.startswith(GENERATED) else (data_dir, False)


def load_dataset(args, train=False, device='cuda', stochastic=False, load=None, foreign=None, finder=None):
    """stochastic: the command line's --mnist_stochastic, never the `mnist_stochastic` that training saved in params.json (`args` is that
    configuration): an existing experiment is evaluated on what it was evaluated on before.  load: who decompresses the test-set file
    (utils/loadz.npz_loader), foreign: who decompresses it when it is not cut at sync markers (utils/loadz.npz_foreign) and finder: which
    block headers the device then looks for (utils/loadz.npz_finder), each handed on only when it was given."""
    data_dir, generated = split_data_dir(args.data_dir)
    if generated and not train:      # make_test_set.py's defaults: seed 42, 100 frames, frame size 64, speed 4
        return MovingMNIST.generated(data_dir, 64, args.nt_cond, args.nt_cond + args.nt_pred, 4, args.n_object, device,
                                     deterministic=not stochastic)
    extra = {} if load is None or train else {'load': load}
    if foreign is not None and not train:
        extra['foreign'] = foreign
    if finder is not None and not train:
        extra['finder'] = finder
    return MovingMNIST.make_dataset(data_dir, 64, args.nt_cond, args.nt_cond + args.nt_pred, 4, not stochastic, args.n_object, train,
                                    device=device, **extra)


def add_stochastic_flag(p):
    """--mnist_stochastic (not in the reference), off by default.  Returns `p`."""
    p.add_argument('--mnist_stochastic', action='store_true',
                   help='Evaluate on the stochastic Moving MNIST variant: the test set is smmnist_test_*.npz (make_test_set.py --stochastic) '
                        'or, with --data_dir generated:D, the stochastic set generated in HBM; swap videos come from the stochastic sampler. '
                        'Only this flag selects it, never the mnist_stochastic saved with the experiment.')
    return p


def test_batches(test_dataset, batch_size):
    """`DataLoader(test_dataset, batch_size)` over the HBM-resident test videos: (cond, target) slices of each batch.  The frames are
    divided by a device scalar: a true division like the reference's host `/ 255` (a Python-number divisor would become a multiplication
    by the reciprocal on the GPU)."""
    data = test_dataset.data
    d255 = torch.tensor(255., dtype=data.dtype, device=data.device)
    nt_cond, seq_len = test_dataset.nt_cond, test_dataset.seq_len
    for start in range(0, data.shape[0], batch_size):
        v = data[start:start + batch_size]
        yield v[:, :nt_cond].div(d255), v[:, nt_cond:seq_len].div(d255)


def main(args):
    compress = savez.npz_compressor()         # who compresses the six frame files: read once, a bad value is refused before any work
    load = loadz.npz_loader()                 # who decompresses the test-set file (VARSEP_NPZ_LOAD): read once, here
    foreign = loadz.npz_foreign()             # and who does when it has no sync markers (VARSEP_NPZ_FOREIGN)
    finder = loadz.npz_finder()               # and which block headers the device then finds (VARSEP_NPZ_FINDER)
    device = setup_device(args)
    seed_all(args.test_seed)
    xp_config = load_xp_config(args, device, args.nt_pred)

    print('Loading data...')
    stochastic = bool(getattr(args, 'mnist_stochastic', False))
    test_dataset = load_dataset(xp_config, train=False, device=device, stochastic=stochastic, load=load, foreign=foreign,
                                **({} if finder == 'dynamic' else {'finder': finder}))
    train_dataset = load_dataset(xp_config, train=True, device=device, stochastic=stochastic)
    nc = 1
    size = 64

    print('Loading model...')
    sep_net = load_model(xp_config, args.epoch)

    print('Generating samples...')
    torch.set_grad_enabled(False)
    nt_test = xp_config.nt_cond + args.nt_pred
    # (the device route converts every batch straight into one buffer per file: the number of test videos is known)
    predictions, content_swap, cond_swap, target_swap, cond, gt = (U8Frames(compress, test_dataset.data.shape[0]) for _ in range(6))
    results = {'mse': [], 'psnr': [], 'ssim': []}
    for x_cond, x_target in test_batches(test_dataset, args.batch_size):
        bsz = len(x_cond)
        cond.append(x_cond)
        gt.append(x_target)

        # Prediction
        x_pred, _, s_code, _ = sep_net.get_forecast(x_cond, nt_test)
        x_pred = x_pred[:, xp_config.nt_cond:]

        # Content swap.  The reference's sequential DataLoader over the training set yields a full batch even when the test batch is
        # ragged; the batch is drawn whole (same NumPy draws) and sliced.  With skip connections the reference hands the already unpacked
        # `s_code` back as init_s_code (model.py:57-62); that is kept as it is.
        x_swap_cond, x_swap_target = train_dataset.batch(args.batch_size)
        x_swap_cond = x_swap_cond[:bsz]
        x_swap_target = x_swap_target[:bsz]
        cond_swap.append(x_swap_cond)
        target_swap.append(x_swap_target)
        x_swap_pred = sep_net.get_forecast(x_swap_cond, nt_test, init_s_code=s_code)[0]
        # reference quirk: `xp_config.dt` is not in params.json and DotDict reads a missing key as None, so this slice keeps all
        # nt_cond + nt_pred frames
        x_swap_pred = x_swap_pred[:, xp_config.dt:]
        content_swap.append(x_swap_pred)

        # Pixelwise quantitative eval
        x_target = x_target.reshape(-1, args.nt_pred, nc, size, size)
        metrics_batch = frame_metrics(x_pred.float().contiguous(), x_target)
        predictions.append(x_pred)
        for name in results:
            results[name].append(metrics_batch[name].cpu())

    results = print_results(results)

    savez.savez_compressed(os.path.join(args.xp_dir, 'results.npz'), results, compress)
    savez.savez_compressed(os.path.join(args.xp_dir, 'predictions.npz'), {'predictions': predictions.cat()}, compress)
    savez.savez_compressed(os.path.join(args.xp_dir, 'gt.npz'), {'gt': gt.cat()}, compress)
    savez.savez_compressed(os.path.join(args.xp_dir, 'cond.npz'), {'cond': cond.cat()}, compress)
    savez.savez_compressed(os.path.join(args.xp_dir, 'content_swap.npz'), {'content_swap': content_swap.cat()}, compress)
    # reference quirk: the swap conditioning frames are stored under the key `target_swap`
    savez.savez_compressed(os.path.join(args.xp_dir, 'cond_swap.npz'), {'target_swap': cond_swap.cat()}, compress)
    savez.savez_compressed(os.path.join(args.xp_dir, 'target_swap.npz'), {'target_swap': target_swap.cat()}, compress)
    return results


def build_parser(stochastic=False):
    """The reference's flags plus --precision; stochastic=True (the command line's parser) adds --mnist_stochastic."""
    p = base_parser('PDE-Driven Spatiotemporal Disentanglement (Moving MNIST testing)', batch_size=16, test_seed=True)
    return add_stochastic_flag(add_precision_flag(p)) if stochastic else add_precision_flag(p)


if __name__ == '__main__':
    main(build_parser(stochastic=True).parse_args())

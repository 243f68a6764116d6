"""Generate tests/golden/smnist_testset.npz by running the REFERENCE's own preprocessing/mnist/make_test_set.py (through runpy, read-only)
with a STOCHASTIC sampler, on the seeded stand-in digits of tests/smnist_testset_inputs.py.

TEST INFRASTRUCTURE ONLY; runs where the reference is:   python tests/make_golden_smnist_testset.py

The script builds its sampler as `MovingMNIST([], frame, 0, seq_len, speed, True, digits, True)`: deterministic=True is written into it, so
the reference cannot write the stochastic file as it stands.  Before the run, `var_sep.data.moving_mnist.MovingMNIST` -- the name the script
imports -- is replaced by a subclass of the reference's class whose constructor passes deterministic=False on; nothing else differs.  The
placeholder `torchvision` / `tqdm` modules are those of tests/make_golden_mmnist_testset.py.  Every line that computes something -- the seed,
the permutation, `_compute_trajectory` with its draws, bounces and redraws, the compositing, the clip, the transpositions, the savez -- is
the reference's own.  The words of the global stream after the script are recorded beside the arrays.  The restatement
tests/smnist_testset_ref.py must reproduce all four arrays and those words for every case before the fixture is written, and every case
must lie inside the walk kernel's budgets (collision passes per step, outputs per trajectory); `windows` must make the kernel slide its
window more than twice.
"""
import importlib
import os
import runpy
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
REF = os.environ.get('VARSEP_REFERENCE', '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import smnist_inputs as SI                 # noqa: E402
import smnist_testset_inputs as I          # noqa: E402
import smnist_testset_ref as R             # noqa: E402
from mmnist_draws_inputs import state_words   # noqa: E402


def run_reference(case, out_dir):
    """The reference's script with a stochastic sampler on the stand-ins of `case`: (the arrays of the file it saved, the stream's words)."""
    images, labels = I.standins(case)

    class MNIST:
        def __init__(self, root, train=True, download=False):
            assert train is False

        def __len__(self):
            return len(images)

        def __getitem__(self, i):
            return images[i], int(labels[i])

    tv = types.ModuleType('torchvision')
    tv.datasets = types.ModuleType('torchvision.datasets')
    tv.datasets.MNIST = MNIST
    tq = types.ModuleType('tqdm')
    tq.trange = range
    sys.modules.update({'torchvision': tv, 'torchvision.datasets': tv.datasets, 'tqdm': tq})
    if REF not in sys.path:
        sys.path.insert(0, REF)
    module = importlib.import_module('var_sep.data.moving_mnist')
    reference_class = module.MovingMNIST

    class Stochastic(reference_class):
        def __init__(self, data, nx, nt_cond, seq_len, max_speed, deterministic, num_digits, train):
            # the script has imported the name by now, and the reference's constructor reaches its base through the module's global
            # `MovingMNIST`, which must be the reference's class again for that
            module.MovingMNIST = reference_class
            super().__init__(data, nx, nt_cond, seq_len, max_speed, False, num_digits, train)

    argv = sys.argv
    sys.argv = ['make_test_set.py', '--data_dir', out_dir, '--seq_len', str(case['seq_len']), '--seed', str(case['seed']), '--digits',
                str(case['digits']), '--frame_size', str(case['frame']), '--max_speed', str(case['speed'])]
    module.MovingMNIST = Stochastic
    try:
        runpy.run_path(os.path.join(REF, 'var_sep', 'preprocessing', 'mnist', 'make_test_set.py'), run_name='__main__')
        words = state_words(np.random)
    finally:
        module.MovingMNIST = reference_class
        sys.argv = argv
    with np.load(os.path.join(out_dir, 'mmnist_test_%ddigits_%d.npz' % (case['digits'], case['frame']))) as z:
        return {k: z[k] for k in I.ARRAYS}, words


def main():
    kept = np.random.get_state()
    out = {'param_names': np.array(I.PARAMS)}
    for name, case in I.CASES.items():
        with tempfile.TemporaryDirectory() as tmp:
            ref, ref_words = run_reference(case, tmp)
        images, labels = I.standins(name)
        watch = SI.Watch(np.random)
        mine, my_words = R.make_test_set(images, labels, case['seed'], case['seq_len'], case['digits'], case['frame'], case['speed'], note=watch)
        for k in I.ARRAYS:
            assert mine[k].dtype == ref[k].dtype and mine[k].shape == ref[k].shape and np.array_equal(mine[k], ref[k]), \
                'tests/smnist_testset_ref.py differs from the reference: %s %s' % (name, k)
            out[name + ':' + k] = ref[k]
        assert np.array_equal(my_words, ref_words), 'tests/smnist_testset_ref.py differs from the reference (stream state): ' + name
        out[name + ':final'] = ref_words
        out[name + ':params'] = np.array([case[k] for k in I.PARAMS], dtype=np.int64)
        # the case lies inside the budgets of the walk kernel, and `windows` is long enough to slide its window more than twice
        assert watch.max_passes <= I.MAX_PASSES and max(watch.outputs) < I.SERIAL_FROM, (name, watch.max_passes, max(watch.outputs))
        if name == 'windows':
            assert sum(watch.outputs) > 2 * I.WINDOW, sum(watch.outputs)
        seq, n_traj = ref['sequences'], len(watch.outputs)
        print('%-8s %s %s, %d clipped pixels; %d outputs over %d trajectories (%.1f each, at most %d), at most %d passes; restatement identical'
              % (name, seq.dtype, seq.shape, int((seq == 255).sum()), sum(watch.outputs), n_traj, sum(watch.outputs) / n_traj,
                 max(watch.outputs), watch.max_passes))
    np.random.set_state(kept)
    np.savez_compressed(I.GOLDEN, **out)
    print('wrote %s (%.1f KB)' % (I.GOLDEN, os.path.getsize(I.GOLDEN) / 1e3))


if __name__ == '__main__':
    main()

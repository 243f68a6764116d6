"""Generate tests/golden/mmnist_testset.npz by running the REFERENCE's own preprocessing/mnist/make_test_set.py (through runpy, read-only
from /root/reference) on the seeded stand-in digits of tests/mmnist_testset_inputs.py.

TEST INFRASTRUCTURE ONLY; runs in the build container:   python tests/make_golden_mmnist_testset.py

The script imports `torchvision.datasets` (to read MNIST) and `tqdm.trange` (a progress bar); neither is installed offline.  Placeholder
modules stand in: `datasets.MNIST(...)` serves the stand-in (image, label) pairs, `trange` is `range`.  Every line that computes something --
the seed, the permutation, `_compute_trajectory` with its draws and bounces, the compositing, the clip, the transpositions, the savez -- is
the reference's own.  The restatement tests/mmnist_testset_ref.py must reproduce all four arrays of every case bit for bit before the
fixture is written.

The geometry without any room (mmnist_testset_inputs.NO_ROOM: a 28 x 28 digit in a 28 x 28 frame) is run too, in a child process under a
time limit, to record that the reference does not finish it (see the note in mmnist_testset_inputs.py); it is not part of the fixture.
"""
import os
import runpy
import subprocess
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

import mmnist_testset_inputs as I      # noqa: E402
import mmnist_testset_ref as R         # noqa: E402

PARAMS = ('images', 'seed', 'seq_len', 'digits', 'frame', 'speed', 'standin_seed')


def run_reference(case, out_dir):
    """The reference's script on the stand-ins of `case`; returns the arrays of the file it saved under out_dir."""
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
    argv = sys.argv
    sys.argv = ['make_test_set.py', '--data_dir', out_dir, '--seq_len', str(case['seq_len']), '--seed', str(case['seed']), '--digits',
                str(case['digits']), '--frame_size', str(case['frame']), '--max_speed', str(case['speed'])]
    try:
        runpy.run_path(os.path.join(REF, 'var_sep', 'preprocessing', 'mnist', 'make_test_set.py'), run_name='__main__')
    finally:
        sys.argv = argv
    with np.load(os.path.join(out_dir, 'mmnist_test_%ddigits_%d.npz' % (case['digits'], case['frame']))) as z:
        return {k: z[k] for k in I.ARRAYS}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--no-room':           # the child process of the time-limit run below
        with tempfile.TemporaryDirectory() as tmp:
            run_reference(I.NO_ROOM, tmp)
        return
    out = {'param_names': np.array(PARAMS)}
    for name, case in I.CASES.items():
        with tempfile.TemporaryDirectory() as tmp:
            ref = run_reference(case, tmp)
        images, labels = I.standins(name)
        mine = R.make_test_set(images, labels, case['seed'], case['seq_len'], case['digits'], case['frame'], case['speed'])
        for k in I.ARRAYS:
            assert mine[k].dtype == ref[k].dtype and mine[k].shape == ref[k].shape and np.array_equal(mine[k], ref[k]), \
                'tests/mmnist_testset_ref.py differs from the reference: %s %s' % (name, k)
            out[name + ':' + k] = ref[k]
        out[name + ':params'] = np.array([case[k] for k in PARAMS], dtype=np.int64)
        seq = ref['sequences']
        print('%-8s %s %s, latents %s %s, %d clipped pixels; restatement identical' % (
            name, seq.dtype, seq.shape, ref['latents'].dtype, ref['latents'].shape, int((seq == 255).sum())))
    np.savez_compressed(I.GOLDEN, **out)
    print('wrote %s (%.1f KB)' % (I.GOLDEN, os.path.getsize(I.GOLDEN) / 1e3))
    try:
        subprocess.run([sys.executable, os.path.abspath(__file__), '--no-room'], timeout=20, check=True, stdout=subprocess.DEVNULL)
        print('NO_ROOM: the reference finished -- make it a case')
    except subprocess.TimeoutExpired:
        print('NO_ROOM: the reference did not finish within 20 s (its bounce loop does not terminate without room)')


if __name__ == '__main__':
    main()

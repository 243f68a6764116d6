"""Inputs of the STOCHASTIC Moving-MNIST test-set fixture (tests/golden/smnist_testset.npz), shared by the fixture generator
(tests/make_golden_smnist_testset.py) and the tests (tests/test_smnist_testset_cpu.py, tests/test_smnist_testset_gpu.py).  Nothing here
imports the reference.

A case is a run of the reference's preprocessing/mnist/make_test_set.py whose sampler was built with deterministic=False (the speed vector
is redrawn from the global stream at every bounce), on the stand-in digits of tests/mmnist_testset_inputs.py: the three geometries of its
CASES, and `windows`, whose 16 trajectories of 100 frames in 4 pixels of room at speed 9 consume several windows of the walk kernel.
"""
import functools
import os

import numpy as np

import mmnist_testset_inputs as M
from mmnist_draws_inputs import N, state_words

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'smnist_testset.npz')
DIGIT = M.DIGIT
ARRAYS = M.ARRAYS
PARAMS = ('images', 'seed', 'seq_len', 'digits', 'frame', 'speed', 'standin_seed')
WINDOW = 4 * N               # outputs the walk kernel holds in LDS at a time (csrc/vs_mmnist_walk_core.h)
SERIAL_FROM = 3 * N          # a trajectory that consumes this many outputs is left to the serial lane
MAX_PASSES = 64              # collision passes per step before the kernel gives up (status 3)

CASES = dict(M.CASES, windows=dict(images=16, seed=11, seq_len=100, digits=2, frame=32, speed=9, standin_seed=5105))

write_t10k = M.write_t10k


def standins(case):
    """(images uint8 [n, 28, 28], labels uint8 [n]) of a case (a name of CASES or a dict of its form): mmnist_testset_inputs' stand-ins."""
    return M.standins(CASES[case] if isinstance(case, str) else case)


@functools.lru_cache(maxsize=None)
def _file():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden(case):
    """{'sequences', 'latents', 'labels', 'digits', 'final'} of a case: the four arrays as the reference wrote them and the words (key[624],
    pos) of the global stream after its script.  Shared and read-only."""
    z = _file()
    params = dict(zip(z['param_names'].tolist(), z[case + ':params'].tolist()))
    assert params == {k: CASES[case][k] for k in params}, (case, params)
    out = {k: z[case + ':' + k] for k in ARRAYS + ('final',)}
    for a in out.values():
        a.setflags(write=False)
    return out


def state_after_permutation(case):
    """(digits_idx, uint32 [625]): the permutation of a case's images and the global stream's words after it -- where the walk starts.  The
    global stream is left as it was found."""
    c = CASES[case]
    kept = np.random.get_state()
    try:
        np.random.seed(c['seed'])
        digits_idx = np.random.permutation(c['images'])
        return digits_idx, state_words(np.random)
    finally:
        np.random.set_state(kept)


def walk_case(case):
    """The case in the form of tests/smnist_inputs.py (compile_host_check / run_host_check and the op's operands): ONE call of n_videos *
    digits trajectories with four prefix draws, from the state after the permutation."""
    c = CASES[case]
    _, words = state_after_permutation(case)
    return dict(name=case, state=words, calls=[(c['images'] // c['digits']) * c['digits']], n_pre=4, starts=None, frame=c['frame'],
                digit=(DIGIT, DIGIT), max_speed=c['speed'], seq_len=c['seq_len'], n_source=c['images'])

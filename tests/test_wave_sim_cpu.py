"""WaveEq generation without a GPU: the parameter and pixel draws, the two preprocessing command lines, the new C entry point's
declaration and argument checks, and the health of the fp64 reference (tests/wave_sim_ref.py) the GPU tests compare the kernel with."""
import ctypes
import os
import re

import numpy as np
import pytest

import wave_sim_ref as R
from spatiotemporal_variable_separation_amd import _lib
from spatiotemporal_variable_separation_amd.preprocessing.wave import gen_pixels, gen_wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# flag -> default of the reference's parsers (preprocessing/wave/gen_wave.py:147-158, gen_pixels.py:29-36); None: required
GEN_WAVE_FLAGS = {'data_dir': None, 'seq_len': 300, 'seed': 42, 'frame_size': 64, 'size': 300, 'dt': 0.001}
GEN_PIXELS_FLAGS = {'data_dir': None, 'number': 100, 'frame_size': 64, 'seed': 42}


def test_wave_parameters_are_the_interleaved_draws():
    np.random.seed(42)
    want = [np.random.uniform(1, 30) if k % 2 == 0 else np.random.uniform(300, 400) for k in range(6)]
    f0, c = gen_wave.wave_parameters(3, 42)
    assert f0.tolist() == want[0::2] and c.tolist() == want[1::2]
    assert f0.dtype == np.float64 and c.dtype == np.float64


def test_gen_pixels_writes_the_two_draws(tmp_path):
    gen_pixels.main(['--data_dir', str(tmp_path)])
    np.random.seed(42)
    rand_w = np.random.randint(64, size=100)
    rand_h = np.random.randint(64, size=100)
    with np.load(tmp_path / 'pixels' / 'pixels.npz') as z:
        assert sorted(z.files) == ['rand_h', 'rand_w']
        assert np.array_equal(z['rand_w'], rand_w) and np.array_equal(z['rand_h'], rand_h)
        assert z['rand_w'].dtype == rand_w.dtype


@pytest.mark.parametrize('module, flags', [(gen_wave, GEN_WAVE_FLAGS), (gen_pixels, GEN_PIXELS_FLAGS)])
def test_parsers_carry_the_reference_flags(module, flags):
    actions = {a.dest: a for a in module.build_parser()._actions}
    for name, default in flags.items():
        assert name in actions, name
        assert actions[name].required == (default is None)
        if default is not None:
            assert actions[name].default == default and type(actions[name].default) is type(default)
    if module is gen_wave:
        assert actions['dt'].type is float and 'type=int' in actions['dt'].help          # the help says why this differs from the reference
        assert module.build_parser().parse_args(['--data_dir', 'x', '--dt', '0.002']).dt == 0.002
        assert set(actions) - set(flags) - {'help'} == {'device'}


def test_gen_wave_refuses_other_frame_sizes_and_a_missing_device(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        gen_wave.main(['--data_dir', str(tmp_path), '--device', '0', '--frame_size', '32'])
    assert e.value.code != 0
    assert '64x64' in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        gen_wave.main(['--data_dir', str(tmp_path)])
    assert e.value.code != 0
    assert '--device' in capsys.readouterr().err
    with pytest.raises(ValueError, match='64x64'):
        gen_wave.generate(2, 32, 5, 0.001, str(tmp_path))
    assert not os.path.exists(tmp_path / 'data')


def test_entry_point_is_declared_bound_and_checks_its_arguments():
    header = open(os.path.join(ROOT, 'include', 'varsep_hip.h')).read()
    assert re.search(r'\bint vs_wave_simulate\(', header)
    assert 'vs_wave_simulate' in _lib.SIGNATURES and 'vs_wave_sim.hip' in _lib.SOURCES
    lib = _lib.load_library()
    assert hasattr(lib, 'vs_wave_simulate')
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for args in ((0, 4, 64, p, p, p, None, p, None, 0, None),          # n_seq = 0
                 (1, 0, 64, p, p, p, None, p, None, 0, None),          # no frame
                 (1, 4, 32, p, p, p, None, p, None, 0, None),          # not a 64x64 frame
                 (1, 4, 64, None, p, p, None, p, None, 0, None),       # null tables
                 (1, 4, 64, p, p, None, None, p, None, 0, None),       # steps without step sizes
                 (1, 4, 64, p, p, p, None, None, None, 0, None)):      # null output
        assert lib.vs_wave_simulate(*args) == -1
        assert 'vs_wave_simulate' in lib.vs_last_error().decode()


def test_source_table_is_the_reference_rounding():
    from spatiotemporal_variable_separation_amd import ops
    source, h = ops.wave_source_table([30.0, 1.0], 7, 0.001)
    t = R.time_grid(7, 0.001)
    assert source.dtype == np.float32 and source.shape == (2, 19) and h.dtype == np.float32 and np.array_equal(h, t[1:] - t[:-1])
    for i in range(6):
        stage = [t[i], t[i] + h[i] * np.float32(1 / 3), t[i] + h[i] * np.float32(2 / 3)]
        assert all(np.asarray(x).dtype == np.float32 for x in stage)
        for k, ts in enumerate(stage):
            assert source[0, 3 * i + k] == R.source_values(30.0, ts) and source[1, 3 * i + k] == R.source_values(1.0, ts)
    assert source[0, 18] == R.source_values(30.0, t[6]) and source[0, 0] == np.float32(30.0)


def test_fp64_reference_stays_bounded_at_the_corner_of_the_parameter_box():
    """f0 = 30, c = 400 (the largest source and the stiffest stencil of U(1, 30) x U(300, 400)), 300 frames: max |w| = 3.2e-3, reached with
    no growth.  A transcription slip in the reference (a stencil weight, a tableau coefficient) shows here as a blow-up."""
    w = R.simulate(30.0, 400.0, 300)
    peak = np.abs(w).reshape(300, -1).max(axis=1)
    assert np.isfinite(w).all() and w.dtype == np.float64
    assert 2.5e-3 < peak.max() < 4e-3
    assert peak[-50:].max() <= peak.max() and peak[-1] < 4e-3
    assert np.all(w[0] == 0)
    border = np.zeros((64, 64), bool)
    border[[0, 1, 62, 63], :] = True
    border[:, [0, 1, 62, 63]] = True
    assert np.all(w[:, border] == 0)                                # from a zero start the outer two rows and columns never move

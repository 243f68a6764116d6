"""CPU: the evaluation CLIs (spatiotemporal_variable_separation_amd.test.*) expose the reference's flags with the same defaults
(recorded from the reference's scripts in tests/golden/eval_cli_flags.json by tests/make_golden_eval_cli.py) and refuse to run
without --device: there is no CPU mode."""
import importlib
import json
import os

import pytest

from golden_util import GOLDEN_DIR

MODULES = {'mnist_test': 'spatiotemporal_variable_separation_amd.test.mnist.test',
           'mnist_test_disentanglement': 'spatiotemporal_variable_separation_amd.test.mnist.test_disentanglement',
           'wave_test': 'spatiotemporal_variable_separation_amd.test.wave.test'}


def _reference_flags():
    with open(os.path.join(GOLDEN_DIR, 'eval_cli_flags.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('script', sorted(MODULES))
def test_parser_has_reference_flags(script):
    parser = importlib.import_module(MODULES[script]).build_parser()
    actions = {a.option_strings[0]: a for a in parser._actions if a.option_strings}
    for flag, default, typ, required in _reference_flags()[script]:
        assert flag in actions, flag
        a = actions[flag]
        assert a.default == default, (flag, a.default, default)
        assert a.required == required, flag
        assert (a.type.__name__ if a.type else None) == typ, flag
    extra = set(actions) - {f[0] for f in _reference_flags()[script]} - {'-h'}
    assert extra == {'--precision'}, extra
    assert actions['--precision'].default == 'fp32' and list(actions['--precision'].choices) == ['fp32', 'bf16']


@pytest.mark.parametrize('script', sorted(MODULES))
def test_cli_refuses_cpu_mode(script, tmp_path):
    mod = importlib.import_module(MODULES[script])
    argv = ['--data_dir', str(tmp_path), '--xp_dir', str(tmp_path)] + ([] if script == 'wave_test' else ['--nt_pred', '5'])
    args = mod.build_parser().parse_args(argv)
    assert args.device is None
    with pytest.raises(RuntimeError, match='no CPU mode'):
        mod.main(args)


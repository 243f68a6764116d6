"""CPU: the shared pieces of the data layer (data/device.py: the device check, the optional reader) and of the evaluation CLIs
(test/utils.py: the params.json block)."""
import json
import os
import types

import numpy as np
import pytest
import torch

from golden_util import install_standin, remove_standin

PKG = 'spatiotemporal_variable_separation_amd'


def test_require_gpu_refuses_the_cpu():
    from spatiotemporal_variable_separation_amd._lib import VarsepHipError
    from spatiotemporal_variable_separation_amd.data.device import require_gpu
    with pytest.raises(VarsepHipError, match='the HBM-resident x set needs an MI355X device; there is no CPU fallback$'):
        require_gpu('x', 'cpu')
    with pytest.raises(VarsepHipError, match=r'no CPU fallback \(see y\)$'):
        require_gpu('x', torch.device('cpu'), hint=' (see y)')
    assert require_gpu('x', None) == torch.device('cuda') and require_gpu('x', 'cuda:1') == torch.device('cuda', 1)


def test_read_optional_native_then_npz_then_hint(tmp_path):
    from spatiotemporal_variable_separation_amd.data.device import optional_module, read_optional
    native, npz = str(tmp_path / 'a.bin'), str(tmp_path / 'a.npz')

    def read():
        return read_optional('varsep_standin_reader', native, npz, lambda m, path: ('native', m.__name__, path),
                             lambda z: ('npz', z['v'].tolist()), 'part', 'CONVERT a.bin')

    with pytest.raises(ValueError) as e:                 # neither file
        read()
    assert str(e.value) == ('%s is missing, and there is no %s.  Where varsep_standin_reader exists, convert each part with\nCONVERT a.bin'
                            % (native, npz))
    open(native, 'wb').close()
    with pytest.raises(ValueError, match='cannot be read: varsep_standin_reader does not import here, and there is no .*\nCONVERT a.bin'):
        read()                                           # a native file nobody can read
    np.savez(npz, v=np.arange(3))
    assert optional_module('varsep_standin_reader') is None and read() == ('npz', [0, 1, 2])
    install_standin('varsep_standin_reader')             # installed after the import of data.device: looked up per call
    try:
        assert read() == ('native', 'varsep_standin_reader', native)
        os.remove(native)
        assert read() == ('npz', [0, 1, 2])              # the module alone does not select the native branch
    finally:
        remove_standin('varsep_standin_reader')
    assert optional_module('varsep_standin_reader') is None


def test_load_xp_config_reads_params_and_overrides(tmp_path):
    from spatiotemporal_variable_separation_amd.test.utils import load_xp_config
    with open(tmp_path / 'params.json', 'w') as f:
        json.dump(dict(nt_cond=3, nt_pred=7, data_dir='/where/it/was/trained', skipco=True), f)
    args = types.SimpleNamespace(xp_dir=str(tmp_path), data_dir='/here', nt_pred=95)
    cfg = load_xp_config(args, 'cuda:0', 40)
    assert (cfg.nt_cond, cfg.skipco, cfg.nt_pred, cfg.data_dir, cfg.xp_dir, cfg.device) == (3, True, 40, '/here', str(tmp_path), 'cuda:0')
    assert cfg.dt is None and args.nt_pred == 95         # a missing key reads as None; the arguments are left alone

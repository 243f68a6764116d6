"""CPU-side checks: the C-ABI library loads and exports every declared symbol, the CLI surface matches the reference,
the product refuses to run without a GPU (no silent CPU fallback), module trees are state-dict compatible."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'varsep_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(vs_[a-z0-9_]+)\s*\(', text)))


def test_library_builds_loads_and_exports_every_declared_symbol():
    from spatiotemporal_variable_separation_amd import _lib
    _lib.build_library()
    lib = _lib.load_library()
    declared = _declared_symbols()
    assert len(declared) >= 25
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/varsep_hip.h but not exported'
        assert name in _lib.SIGNATURES, f'{name} has no ctypes signature'
    assert set(_lib.SIGNATURES) == set(declared)
    assert lib.vs_version().decode().startswith('varsep_hip')
    assert lib.vs_gemm_workspace_bytes(128, 1200, 20480) > 0        # host-side planning only, no GPU call
    assert lib.vs_gemm_workspace_bytes(4096, 4096, 4096) == 0


def test_argument_errors_are_reported_not_thrown():
    from spatiotemporal_variable_separation_amd import _lib
    lib = _lib.load_library()
    rc = lib.vs_gemm(0, -1, 4, 4, None, 4, 0, None, 4, 0, None, 4, 0, 1.0, None, 0, None, 0, 0, 0, 0, None, 0, None)
    assert rc == -1 and b'vs_gemm' in lib.vs_last_error()


def test_product_refuses_cpu_tensors():
    from spatiotemporal_variable_separation_amd import _lib
    from spatiotemporal_variable_separation_amd.networks.factory import build_sep_net
    from oracle.golden_configs import CONFIGS, make_batch
    for name in ('mlp_mul', 'dcgan_tiny'):
        cfg = CONFIGS[name]
        net = build_sep_net(cfg)
        cond, _ = make_batch(cfg)
        with pytest.raises(_lib.VarsepHipError, match='no CPU fallback'):
            net.get_forecast(cond, 3)


def test_state_dict_layout_matches_reference_compatible_oracle():
    from oracle import cpu_ref
    from oracle.golden_configs import CONFIGS
    from spatiotemporal_variable_separation_amd.networks.factory import build_sep_net
    for name, cfg in CONFIGS.items():
        a, b = build_sep_net(cfg).state_dict(), cpu_ref.build_sep_net(cfg).state_dict()
        assert list(a.keys()) == list(b.keys()), name
        for k in a:
            assert a[k].shape == b[k].shape, (name, k)


def test_cli_matches_reference_surface():
    from spatiotemporal_variable_separation_amd.options import parser
    # README recipes of the reference, including the `--gain_res` abbreviation of the SST recipe (README.md:86)
    args = parser.parse_args('--xp_dir x --data_dir d --data sst --nt_cond 4 --nt_pred 6 --epochs 30 --code_size_t 64 '
                             '--code_size_s 196 --gain_res 0.2 --offset 0 --gain_resnet 0.71 --architecture encoderSST '
                             '--decoder_architecture decoderSST --lamb_ae 1 --lamb_s 100 --lamb_t 5e-6 --skipco '
                             '--n_blocks 2'.split())
    assert args.gain_resnet == 0.71 and args.skipco and args.n_blocks == 2 and args.offset == 0
    d = parser.parse_args('--xp_dir x --data_dir d'.split())
    assert (d.nt_cond, d.nt_pred, d.code_size_s, d.code_size_t, d.batch_size, d.lr, d.offset) == (5, 10, 128, 20, 128, 4e-4, 5)
    assert (d.lamb_ae, d.lamb_s, d.lamb_t, d.lamb_pred, d.beta1, d.beta2) == (10, 45, 0.001, 45, 0.9, 0.99)
    assert d.architecture == 'dcgan' and d.mixing == 'concat' and d.res_hidden_size == 512 and d.gain_resnet == 1.41
    with pytest.raises(SystemExit):
        parser.parse_args('--xp_dir x --data_dir d --torch_amp --apex_amp'.split())


def test_factory_asserts_like_reference():
    from spatiotemporal_variable_separation_amd.networks.factory import get_decoder, get_encoder
    with pytest.raises(AssertionError):
        get_decoder('mlp', [1, 8, 8], 4, 6, 'sigmoid', 8, 3, 'mul', False, 'normal', 0.02)      # mul needs equal codes
    with pytest.raises(AssertionError):
        get_decoder('mlp', [1, 8, 8], 4, 4, 'sigmoid', 8, 3, 'concat', True, 'normal', 0.02)    # skipco needs conv decoder
    with pytest.raises(AssertionError):
        get_encoder('dcgan', [1, 32, 32], 8, 4, 3, 2, 'normal', 0.02)                             # dcgan is 64x64 only


def test_init_net_statistics():
    from spatiotemporal_variable_separation_amd.networks.factory import get_resnet, get_encoder
    torch.manual_seed(0)
    r = get_resnet(8, 1, 64, 'orthogonal', 1.41)
    w = r.blocks[0].mlp.module[0][0].weight             # [64, 8] orthogonal columns scaled by the gain
    assert torch.allclose(w.t() @ w, 1.41 ** 2 * torch.eye(8), atol=1e-4)
    e = get_encoder('mlp', [1, 8, 8], 4, 256, 3, 2, 'normal', 0.02)
    assert abs(e.mlp.module[1][1].weight.std().item() - 0.02) < 2e-3 and e.mlp.module[1][1].bias.abs().max() == 0


def test_reference_written_checkpoints_load_without_the_reference_package():
    """The four files the REFERENCE's `save` wrote (tests/golden/ckpt_*: whole-module pickles of var_sep.networks.* classes,
    oracle/make_golden_ckpt.py) unpickle into this package's classes with `var_sep` absent, and carry the weights they were saved with."""
    import os
    import sys
    import torch
    from oracle import cpu_ref
    from oracle.golden_configs import CONFIGS, fill_net
    from spatiotemporal_variable_separation_amd.networks.factory import build_sep_net
    from spatiotemporal_variable_separation_amd.utils.helper import load_model, load_sep_net
    assert not any(m == 'var_sep' or m.startswith('var_sep.') for m in sys.modules)
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    for name in ('mlp_mul', 'dcgan_tiny', 'dcgan_skip_mul', 'vgg32_tiny'):
        cfg = CONFIGS[name]
        blob = open(os.path.join(root, 'ckpt_' + name, 'ov_Et.pt'), 'rb').read()
        assert b'var_sep.networks' in blob                      # really a reference pickle
        want = fill_net(cpu_ref.build_sep_net(cfg), cfg).state_dict()
        net = load_model(os.path.join(root, 'ckpt_' + name), build_sep_net(cfg))
        got = net.state_dict()
        assert set(got) == set(want)
        assert all(torch.equal(got[k], want[k]) for k in want), name
        whole = load_sep_net(os.path.join(root, 'ckpt_' + name), cfg['nt_cond'], bool(cfg.get('skipco', False)))
        assert not whole.training
        for part in (whole.Es, whole.Et, whole.decoder, whole.t_resnet):
            assert type(part).__module__.startswith('spatiotemporal_variable_separation_amd.networks.')
        assert all(torch.equal(v, want[k]) for k, v in whole.state_dict().items())
    assert not any(m == 'var_sep' or m.startswith('var_sep.') for m in sys.modules)


def test_bench_line_is_short_and_parses():
    """The driver reads an 8 KB tail of stdout: the ONE result line must stay under 4 KB whatever the full result holds (round 3's
    22.5 KB line went unparsed).  Canned full result = the round-3 line itself, every workload with five roofline groups and prose."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    saved = {k: os.environ.get(k) for k in ('GPU_MAX_HW_QUEUES', 'VARSEP_PACKAGE_SET')}
    try:
        spec.loader.exec_module(bench)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    full = json.load(open(os.path.join(ROOT, 'profiles', 'r03_bench_default.json')))
    assert len(json.dumps(full)) > 20000
    full['configs']['broken'] = {'error': 'RuntimeError: ' + 'x' * 300}
    line = bench.compact_line(full)
    assert len(line) < 4096 and '\n' not in line
    back = json.loads(line)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data'):
        assert back[k] == full[k], k
    assert back['config']['workload'] == full['config']['workload']
    for k in ('kernel', 'bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
        assert back['roofline'][k] == full['roofline'][k], k
    for k in ('value', 'unit', 'cores', 'kind', 'sample'):
        assert back['cpu_baseline'][k] == full['cpu_baseline'][k], k
    assert set(back['configs']) == set(full['configs'])
    assert back['configs']['sst_fp16']['ms_per_step'] == full['configs']['sst_fp16']['ms_per_step']
    assert back['configs']['sst']['roofline']['kernel'] == full['configs']['sst']['roofline']['kernel']
    # a pathologically long result still fits (optional fields are shed)
    full['cpu_baseline']['sample'] = 'y' * 5000
    assert len(bench.compact_line(full)) < 4096


def test_profile_tables_are_tied_to_the_sources():
    from spatiotemporal_variable_separation_amd.profiling import source_sha
    a = source_sha()
    assert len(a) == 16 and a == source_sha()


def test_fp32_split_pieces_reconstruct_the_value_and_six_products_the_convolution():
    """ops._split16 / _SPLIT_TERMS (VARSEP_FP32_SPLIT, the route that runs fp32 steps on the 16-bit convolution kernels): three bf16 pieces
    carry an fp32 value exactly, and the six leading piece products of a bilinear map -- each evaluated like the kernels do: bf16 operands,
    exact products, fp32 accumulation -- reproduce the fp32 result to fp32 rounding (two pieces / three products would leave 2^-16)."""
    import torch
    import torch.nn.functional as F
    from spatiotemporal_variable_separation_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn((4, 24, 12, 12), generator=g) * torch.logspace(-3, 2, 24).view(1, 24, 1, 1)
    w = torch.randn((16, 24, 3, 3), generator=g) * 0.05
    xs, ws = ops._split16(x), ops._split16(w)
    assert all(p.dtype == torch.bfloat16 for p in xs + ws)
    assert torch.equal(xs[0].float() + xs[1].float() + xs[2].float(), x)
    assert torch.equal(ws[0].float() + ws[1].float() + ws[2].float(), w)
    ref = F.conv2d(x.double(), w.double(), padding=1)
    six = sum(F.conv2d(xs[i].double(), ws[j].double(), padding=1) for i, j in ops._SPLIT_TERMS)       # products of bf16 values are exact
    three = sum(F.conv2d(xs[i].double(), ws[j].double(), padding=1) for i, j in ((0, 0), (0, 1), (1, 0)))
    e6 = ((six - ref).norm() / ref.norm()).item()
    e3 = ((three - ref).norm() / ref.norm()).item()
    assert e6 < 2e-7 and e3 > 20 * e6, (e6, e3)


def _switches_read_by_the_package():
    """Every VARSEP_* / VS_* name the package reads from the environment: os.environ.get / os.environ[...] / `in os.environ` / os.getenv in its
    Python, getenv("...") in csrc/."""
    import glob
    pkg = os.path.join(ROOT, 'spatiotemporal_variable_separation_amd')
    name = r'''['"]((?:VARSEP|VS)_[A-Z0-9_]+)['"]'''
    py = [r'environ\.get\(\s*' + name, r'environ\[\s*' + name + r'\s*\]', name + r'\s+(?:not\s+)?in\s+\w*\.?environ\b', r'getenv\(\s*' + name]
    found = set()
    for path in glob.glob(os.path.join(pkg, '**', '*.py'), recursive=True):
        text = open(path).read()
        for pat in py:
            found.update(re.findall(pat, text))
    for path in glob.glob(os.path.join(pkg, 'csrc', '*.hip')) + glob.glob(os.path.join(pkg, 'csrc', '*.h')):
        found.update(re.findall(r'getenv\(\s*"((?:VARSEP|VS)_[A-Z0-9_]+)"', open(path).read()))
    return found


def test_every_environment_switch_is_in_the_integration_table():
    """INTEGRATION.md, section "Environment switches", has one row per switch the package reads, and no row for a switch nothing reads: a new
    switch needs a row (name, where it is read, values, default, who uses it), a retired one loses its row."""
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    m = re.search(r'^## Environment switches\n(.*?)(?=^## |\Z)', text, flags=re.S | re.M)
    assert m, 'INTEGRATION.md has no section "Environment switches"'
    rows = re.findall(r'^\|\s*`((?:VARSEP|VS)_[A-Z0-9_]+)`\s*\|', m.group(1), flags=re.M)
    assert len(rows) == len(set(rows)), sorted(r for r in set(rows) if rows.count(r) > 1)
    read = _switches_read_by_the_package()
    assert len(read) >= 30
    assert set(rows) == read, {'read but not in the table': sorted(read - set(rows)), 'in the table but not read': sorted(set(rows) - read)}

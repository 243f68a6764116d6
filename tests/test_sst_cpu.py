"""CPU: the host half of the SST data path (data/sst.py: `build_zones`, `item_table`) against the reference's own datasets on the synthetic
zones of tests/sst_inputs.py (tests/golden/sst/dataset.npz, written by tests/make_golden_sst.py), its error cases, the new C entry point's
declaration, `main.load_dataset`, and the evaluation CLI's flags against the reference script's (tests/golden/sst/eval_cli/flags.json)."""
import json
import os
import shutil

import numpy as np
import pytest

import sst_inputs as I

PKG = 'spatiotemporal_variable_separation_amd'


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return I.write_tree(str(tmp_path_factory.mktemp('sst')))


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(I.GOLDEN, 'dataset.npz')) as z:
        return {k: z[k] for k in z.files}


def _check_against_golden(data_dir, golden):
    from spatiotemporal_variable_separation_amd.data.sst import build_zones, item_table
    for call, kw in I.CALLS.items():
        zones, nc, npred = kw['zones'], kw['nt_cond'], kw['nt_pred']
        frames, consts, zone_range, L = build_zones(data_dir, zones)
        assert L == I.L and frames.dtype == np.float32 and frames.shape == (len(zones) * L, 64 * 64) and frames.flags.c_contiguous
        assert consts.dtype == np.float32 and consts.shape == (len(zones) * L, 4)
        assert zone_range.dtype == np.float32 and zone_range.shape == (len(zones), 2)
        first, len_ = item_table(len(zones), L, nc, npred, kw['train'])
        assert first.dtype == np.int32 and len(first) == len(zones) * len_ == int(golden['len_%s' % call])
        assert first.min() >= 0 and int(first.max()) + nc + npred <= len(frames)                 # every window stays inside the timeline
        items = I.assemble(frames, first, np.arange(len(first)), nc + npred)
        assert np.array_equal(I.item_crcs(items), golden['crc_%s' % call]), call
        for c, index in I.WHOLE_ITEMS:
            if c == call:
                want, got = golden[I.whole_item_key(c, index)], items[index]
                assert got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (c, index)
        # the constants of every item's target days, the zone of every item and the zones' ranges
        day0 = first.astype(np.int64) + nc
        got_consts = consts[day0[:, None] + np.arange(npred)[None]]
        want_consts = golden['const_%s' % call]
        assert got_consts.shape == want_consts.shape and np.array_equal(got_consts.view(np.uint32), want_consts.view(np.uint32)), call
        assert np.array_equal(np.asarray(zones)[np.arange(len(first)) // len_], golden['file_id_%s' % call])
        assert np.array_equal(zone_range, golden['range_%s' % call].astype(np.float32))
        if not kw['train']:                              # the last test window ends exactly on the zone's last day
            assert int(first[len_ - 1]) + nc + npred == L and int(first[0]) == int(0.8 * L) + 2
    return True


def test_build_zones_matches_reference_items(tree, golden):
    assert _check_against_golden(tree, golden)


def test_build_zones_through_netcdf4(tmp_path, golden):
    """The .nc branch, through a stand-in netCDF4 that delivers masked arrays: same frames, constants and items."""
    data_dir = I.touch_nc_tree(str(tmp_path))
    I.install_fake_netcdf4()
    try:
        assert _check_against_golden(data_dir, golden)
    finally:
        I.remove_fake_netcdf4()


def test_both_promotions_occur_and_round_once(tree):
    """A float64 climatology makes the whole zone float64 before the one rounding to fp32: normalising zone 2 in fp32 gives other bits."""
    from spatiotemporal_variable_separation_amd.data.sst import build_zones
    arrays = I.arrays()
    assert arrays[1]['daily_mean'].dtype == np.float32 and arrays[2]['daily_mean'].dtype == np.float64
    frames = build_zones(tree, [2])[0]
    z = arrays[2]
    th = (z['thetao'] - z['daily_mean'].reshape(-1, 1, 1)) / z['daily_std'].reshape(-1, 1, 1)
    assert th.dtype == np.float64
    th = (th - th.mean(axis=(1, 2)).reshape(-1, 1, 1)) / th.std(axis=(1, 2)).reshape(-1, 1, 1)
    assert np.array_equal(frames, th.astype(np.float32).reshape(I.L, -1))
    low = {k: v.astype(np.float32) for k, v in z.items()}
    t32 = (low['thetao'] - low['daily_mean'].reshape(-1, 1, 1)) / low['daily_std'].reshape(-1, 1, 1)
    t32 = (t32 - t32.mean(axis=(1, 2)).reshape(-1, 1, 1)) / t32.std(axis=(1, 2)).reshape(-1, 1, 1)
    assert t32.dtype == np.float32 and not np.array_equal(frames, t32.reshape(I.L, -1))


def test_missing_zone_file_names_the_conversion(tree, tmp_path):
    from spatiotemporal_variable_separation_amd.data.sst import build_zones
    part = str(tmp_path / 'part')
    os.makedirs(part)
    for zone in (17, 18, 20):
        shutil.copy(os.path.join(tree, I.NPZ_NAME.format(zone)), part)
    with pytest.raises(ValueError) as e:
        build_zones(part, range(17, 21))
    text = str(e.value)
    assert I.NC_NAME.format(19) in text and I.NPZ_NAME.format(19) in text and len(text.splitlines()) == 3
    assert 'netCDF4.Dataset(' in text and 'np.savez(' in text and "v['thetao'][:].data" in text and "daily_std=v['daily_std'][:].data" in text
    readme = open(os.path.join(os.path.dirname(I.HERE), 'README.md')).read()
    assert "daily_std=v['daily_std'][:].data" in readme                          # the README states the same conversion
    # an .nc file without an importable netCDF4 is the same error
    open(os.path.join(part, I.NC_NAME.format(19)), 'wb').close()
    with pytest.raises(ValueError, match='netCDF4 does not import'):
        build_zones(part, range(17, 21))


def test_zones_of_unequal_length_raise(tmp_path):
    from spatiotemporal_variable_separation_amd.data.sst import build_zones
    arrays = dict(I.arrays())
    arrays[18] = {k: v[:-1] for k, v in arrays[18].items()}
    data_dir = I.write_tree(str(tmp_path), zones=(17, 18), zone_arrays=arrays)
    with pytest.raises(ValueError, match='unequal length'):
        build_zones(data_dir, [17, 18])
    assert build_zones(data_dir, [18])[3] == I.L - 1
    with pytest.raises(ValueError):
        build_zones(data_dir, [])


def test_a_half_too_short_for_one_window_raises():
    from spatiotemporal_variable_separation_amd.data.sst import half_bounds, item_table
    assert half_bounds(120, 2, 10, False) == (96, 11) and half_bounds(120, 2, 10, True) == (0, 83)
    assert half_bounds(120, 4, 18, False) == (96, 1)          # one window: days 98 .. 119
    with pytest.raises(ValueError, match='too short'):
        half_bounds(120, 4, 19, False)
    with pytest.raises(ValueError, match='too short'):
        item_table(3, 20, 4, 11, True)                        # int(0.8 * 20) = 16 days < 4 + 11 + 1 + 1
    first, len_ = item_table(2, 120, 4, 18, False)
    assert len_ == 1 and first.tolist() == [98, 218]


def test_header_declares_and_library_exports_the_sst_metrics():
    from spatiotemporal_variable_separation_amd import _lib
    root = os.path.dirname(I.HERE)
    assert 'int vs_sst_frame_metrics(' in open(os.path.join(root, 'include', 'varsep_hip.h')).read()
    _lib.build_library()
    assert hasattr(_lib.load_library(), 'vs_sst_frame_metrics') and 'vs_sst_frame_metrics' in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['vs_sst_frame_metrics'][1]) == 19


def test_load_dataset_has_the_sst_branch(tmp_path):
    """`main.load_dataset` reaches data/sst.py for --data sst: on an empty directory the error is the loader's ValueError with the
    conversion hint, no longer NotImplementedError."""
    from spatiotemporal_variable_separation_amd.main import load_dataset
    from spatiotemporal_variable_separation_amd.options import parser
    args = parser.parse_args(['--xp_dir', str(tmp_path), '--data_dir', str(tmp_path), '--data', 'sst', '--nt_cond', '4', '--nt_pred', '6',
                              '--zones', '3', '5'])
    assert args.zones == [3, 5]
    with pytest.raises(ValueError, match=r'data_3\.nc is missing'):
        load_dataset(args, device='cuda:0')
    args.data = 'no_such_set'
    with pytest.raises(NotImplementedError, match='SST'):
        load_dataset(args, device='cuda:0')


def test_parser_has_reference_flags():
    from spatiotemporal_variable_separation_amd.test.sst import test as cli
    with open(os.path.join(I.GOLDEN, 'eval_cli', 'flags.json')) as f:
        flags = json.load(f)
    assert [f[0] for f in flags] == ['--data_dir', '--xp_dir', '--epoch', '--device']
    actions = {a.option_strings[0]: a for a in cli.build_parser()._actions if a.option_strings}
    for flag, default, typ, required in flags:
        a = actions[flag]
        assert a.default == default and a.required == required and (a.type.__name__ if a.type else None) == typ, flag
    assert set(actions) - {f[0] for f in flags} - {'-h'} == {'--batch_size', '--precision'}
    assert actions['--precision'].default == 'fp32' and actions['--batch_size'].type is int


def test_cli_refuses_cpu_mode(tmp_path):
    from spatiotemporal_variable_separation_amd.test.sst import test as cli
    args = cli.build_parser().parse_args(['--data_dir', str(tmp_path), '--xp_dir', str(tmp_path)])
    assert args.device is None
    with pytest.raises(RuntimeError, match='no CPU mode'):
        cli.main(args)

"""CPU: the host half of the TaxiBJ data path (data/taxibj.py: `build_windows`) against the reference's own datasets on the synthetic
years of tests/taxibj_inputs.py (tests/golden/taxibj/dataset.npz, written by tests/make_golden_taxibj.py), its error cases, and the
evaluation CLI's flags against the reference script's (tests/golden/taxibj/eval_cli/flags.json)."""
import json
import os

import numpy as np
import pytest

import taxibj_inputs as I

PKG = 'spatiotemporal_variable_separation_amd'


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return I.write_tree(str(tmp_path_factory.mktemp('taxibj')))


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(I.GOLDEN, 'dataset.npz')) as z:
        return {k: z[k] for k in z.files}


def _check_against_golden(data_dir, golden):
    from spatiotemporal_variable_separation_amd.data.taxibj import build_windows
    for call, kw in I.CALLS.items():
        frames, first, n_train, mmn = build_windows(data_dir, len_closeness=kw['len_closeness'], len_test=kw['len_test'])
        L = kw['len_closeness']
        assert frames.dtype == np.float32 and frames.ndim == 2 and frames.shape[1] == 2 * 32 * 32 and frames.flags.c_contiguous
        assert first.dtype == np.int32 and first.ndim == 1
        assert [n_train, len(first) - n_train] == golden['len_%s' % call].tolist()
        assert float(mmn._min) == float(golden['min_%s' % call]) and float(mmn._max) == float(golden['max_%s' % call])
        assert first.min() >= L - 1 and first.max() < len(frames)                 # every window stays inside the timeline
        halves = {'train': np.arange(n_train), 'test': np.arange(n_train, len(first))}
        items = {half: I.assemble(frames, first, idx, L) for half, idx in halves.items()}
        for half in halves:
            assert np.array_equal(I.item_crcs(items[half]), golden['crc_%s_%s' % (call, half)]), (call, half)
        for c, half, index in I.WHOLE_ITEMS:
            if c == call:
                want = golden[I.whole_item_key(c, half, index)]
                got = items[half][index]
                assert got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (c, half, index)
    assert float(items['test'].max()) == 1.0            # call b: the fit saw the large values
    return True


def test_build_windows_matches_reference_items(tree, golden):
    assert _check_against_golden(tree, golden)
    from spatiotemporal_variable_separation_amd.data.taxibj import build_windows
    frames, first, n_train, _ = build_windows(tree, len_closeness=8)                # the defaults of make_datasets: call a
    assert n_train == 192 and len(first) == 1536 and len(frames) == 1584
    assert frames.max() > 1.0 and frames[:len(frames) - 1344].max() == 1.0 and frames.min() == 0.0


def test_build_windows_through_h5py(tmp_path, golden):
    """The .h5 branch, through a stand-in h5py that delivers bytes timestamps: same frames, table and items."""
    data_dir = I.touch_h5_tree(str(tmp_path))
    I.install_fake_h5py()
    try:
        assert _check_against_golden(data_dir, golden)
    finally:
        I.remove_fake_h5py()


def test_npz_and_h5py_trees_give_identical_arrays(tree, tmp_path):
    from spatiotemporal_variable_separation_amd.data.taxibj import build_windows
    a = build_windows(tree, len_closeness=6, len_test=100)
    data_dir = I.touch_h5_tree(str(tmp_path))
    I.install_fake_h5py()
    try:
        b = build_windows(data_dir, len_closeness=6, len_test=100)
    finally:
        I.remove_fake_h5py()
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_frames_do_not_depend_on_the_files_dtype(tmp_path, tree):
    """Counts stored as int32 give the bits float64 files give: the normalisation runs in the dtype NumPy gives the reference's expression
    (float64 for both) and is rounded to fp32 once."""
    from spatiotemporal_variable_separation_amd.data.taxibj import build_windows
    ints = {year: (data.astype(np.int32), date) for year, (data, date) in I.arrays().items()}
    data_dir = I.touch_h5_tree(str(tmp_path))
    I.install_fake_h5py(ints)
    try:
        got = build_windows(data_dir, len_closeness=8)
    finally:
        I.remove_fake_h5py()
    want = build_windows(tree, len_closeness=8)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])


def _tree_with(tmp_path, year, edit):
    """An h5py stand-in tree whose `year` has its (data, date) replaced by edit(data, date)."""
    arrays = dict(I.arrays())
    arrays[year] = edit(*arrays[year])
    data_dir = I.touch_h5_tree(str(tmp_path))
    I.install_fake_h5py(arrays)
    return data_dir


def test_unsorted_timestamps_raise(tmp_path):
    from spatiotemporal_variable_separation_amd.data.taxibj import build_windows

    def swap(data, date):                                # slots 10 and 11 of day 1 exchanged: the day still starts at 1 and ends at 48
        date = list(date)
        date[48 + 9], date[48 + 10] = date[48 + 10], date[48 + 9]
        return data, date

    data_dir = _tree_with(tmp_path, 15, swap)
    try:
        with pytest.raises(ValueError, match='unsorted or duplicated'):
            build_windows(data_dir, len_closeness=8)
    finally:
        I.remove_fake_h5py()


def test_duplicated_timestamps_raise(tmp_path):
    from spatiotemporal_variable_separation_amd.data.taxibj import build_windows

    def duplicate(data, date):                           # day 1 holds slot 5 twice and no slot 6: 48 entries from 1 to 48, so the day is kept
        date = list(date)
        date[48 + 5] = date[48 + 4]
        return data, date

    data_dir = _tree_with(tmp_path, 15, duplicate)
    try:
        with pytest.raises(ValueError, match='unsorted or duplicated'):
            build_windows(data_dir, len_closeness=8)
    finally:
        I.remove_fake_h5py()


def test_missing_year_file_names_the_conversion(tree, tmp_path):
    import shutil
    from spatiotemporal_variable_separation_amd.data.taxibj import build_windows
    part = str(tmp_path / 'part')
    os.makedirs(part)
    for year in (13, 14, 16):
        shutil.copy(os.path.join(tree, I.NPZ_NAME.format(year)), part)
    with pytest.raises(ValueError) as e:
        build_windows(part, len_closeness=8)
    text = str(e.value)
    assert I.H5_NAME.format(15) in text and I.NPZ_NAME.format(15) in text
    assert 'h5py.File(' in text and 'np.savez(' in text and "f['data'][()]" in text and "f['date'][()]" in text
    readme = open(os.path.join(os.path.dirname(I.HERE), 'README.md')).read()
    assert "np.savez(" in readme and "date=f['date'][()]" in readme            # the README states the same conversion
    # an .h5 file without an importable h5py is the same error
    open(os.path.join(part, I.H5_NAME.format(15)), 'wb').close()
    with pytest.raises(ValueError, match='h5py'):
        build_windows(part, len_closeness=8)


@pytest.mark.parametrize('len_test', [1536, 5000])
def test_len_test_of_at_least_the_window_count_leaves_an_empty_train_set(tree, len_test):
    from spatiotemporal_variable_separation_amd.data.taxibj import build_windows
    if len_test >= 1584:                                 # `[:-len_test]` of the FRAMES is empty as well: NumPy cannot fit a minimum
        with pytest.raises(ValueError):
            build_windows(tree, len_closeness=8, len_test=len_test)
        return
    frames, first, n_train, _ = build_windows(tree, len_closeness=8, len_test=len_test)
    assert n_train == 0 and len(first) == 1536


def test_timestamps_parse_with_integer_arithmetic():
    from spatiotemporal_variable_separation_amd.data.taxibj import timestamp_minutes
    a = timestamp_minutes(b'2015022848')                 # 23:30 on 28 February
    assert timestamp_minutes('2015030101') - a == 30 and timestamp_minutes('2015022847') == a - 30
    assert timestamp_minutes(b'2016010101') - timestamp_minutes(b'2015123148') == 30
    assert timestamp_minutes('2013070103') - timestamp_minutes('2013070101') == 60
    with pytest.raises(ValueError):
        timestamp_minutes('2013070149')


def test_minmax_normalization_surface():
    from spatiotemporal_variable_separation_amd.data.taxibj import MinMaxNormalization
    m = MinMaxNormalization()
    x = np.array([[2.0, 4.0], [10.0, 6.0]])
    m.fit(x)
    assert (m._min, m._max) == (2.0, 10.0)
    y = m.transform(x)
    assert np.array_equal(y, 1. * (x - 2.0) / 8.0) and np.array_equal(m.inverse_transform(y), x)


def test_parser_has_reference_flags():
    from spatiotemporal_variable_separation_amd.test.taxibj import test as cli
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
    from spatiotemporal_variable_separation_amd.test.taxibj import test as cli
    args = cli.build_parser().parse_args(['--data_dir', str(tmp_path), '--xp_dir', str(tmp_path)])
    assert args.device is None
    with pytest.raises(RuntimeError, match='no CPU mode'):
        cli.main(args)


def test_header_declares_and_library_exports_the_gather():
    from spatiotemporal_variable_separation_amd import _lib
    root = os.path.dirname(I.HERE)
    assert 'int vs_gather_timeline(' in open(os.path.join(root, 'include', 'varsep_hip.h')).read()
    _lib.build_library()
    assert hasattr(_lib.load_library(), 'vs_gather_timeline') and 'vs_gather_timeline' in _lib.SIGNATURES

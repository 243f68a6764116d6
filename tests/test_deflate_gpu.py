"""GPU: vs_deflate_chunks / vs_deflate_pack / vs_crc32 (csrc/vs_deflate.hip) through ops.deflate_raw and ops.crc32 on the corpus of
tests/deflate_inputs.py -- against zlib's inflate, against the host build of the same logic (byte for byte), against the device's own
inflate kernel, with guard bytes round the slots -- and the Moving-MNIST test file written with VARSEP_NPZ_COMPRESS=device."""
import os
import zlib

import numpy as np
import pytest
import torch

import deflate_inputs as D
import mmnist_testset_inputs as MI
from guard_util import CANARY, guarded_ops
from spatiotemporal_variable_separation_amd import _lib, ops
from spatiotemporal_variable_separation_amd.preprocessing.mnist import make_test_set

pytestmark = pytest.mark.gpu

NAMES = [name for name, _ in D.corpus()]


def _device_source(name, a):
    """The input on the device; the inputs of SOURCE_OFFSET start 1 and 3 bytes into their allocation."""
    off = D.SOURCE_OFFSET.get(name, 0)
    buf = torch.empty(a.size + off, dtype=torch.uint8, device='cuda')
    buf[off:] = torch.from_numpy(a.copy())
    t = buf[off:]
    assert t.data_ptr() % 4 == off % 4 and t.is_contiguous()
    return t


@pytest.fixture(scope='module')
def compressed():
    """{name: (array, packed bytes, n_chunks)}: every input of the corpus through ops.deflate_raw, once."""
    out = {}
    for name, a in D.corpus():
        packed, n_chunks = ops.deflate_raw(_device_source(name, a))
        assert packed.dtype == torch.uint8 and packed.is_cuda and packed.dim() == 1
        out[name] = (a, packed.cpu().numpy().tobytes(), n_chunks)
    return out


def _inflate_raw(stream):
    d = zlib.decompressobj(-15)
    out = d.decompress(stream)
    assert d.eof and not d.unused_data
    return out


@pytest.mark.parametrize('name', NAMES)
def test_zlib_inflates_the_kernels_stream_to_the_input(name, compressed):
    a, packed, n_chunks = compressed[name]
    assert n_chunks == -(-a.size // D.L)
    assert _inflate_raw(packed + D.FINAL_BLOCK) == a.tobytes()
    assert len(packed) + len(D.FINAL_BLOCK) <= D.bound(a.size)
    assert 5 * n_chunks <= len(packed) and (n_chunks == 0 or packed[-4:] == b'\x00\x00\xff\xff')


def test_kernel_bytes_equal_the_host_builds(compressed, tmp_path):
    exe, sanitized = D.compile_host_check(tmp_path)
    records, stdout = D.run_host_check(exe, [a for _, a in D.corpus()], tmp_path)
    assert stdout.strip().splitlines()[-1].endswith('mismatches 0'), stdout[-2000:]
    for (name, _), rec in zip(D.corpus(), records):
        _, packed, n_chunks = compressed[name]
        assert n_chunks == rec['n_chunks'] and len(packed) == len(rec['stream']) and packed == rec['stream'], name


def test_sizes_stay_below_the_bound_and_nothing_is_written_past_them():
    """The entry point itself, with the tightest slots it accepts and 0xFF everywhere: bytes of a slot behind sizes[c] stay untouched."""
    lib = _lib.load_library()
    c = dict(D.corpus())
    for name, chunk in (('random_40000', D.L), ('fibonacci', D.L), ('3L_plus_5', 4096), ('all_256', ops.DEFLATE_MIN_CHUNK), ('zeros_300k', D.L)):
        a = c[name]
        src = torch.from_numpy(a.copy()).cuda()
        stride = chunk + ops.DEFLATE_SLOT_EXTRA
        n_chunks = -(-a.size // chunk)
        slots = torch.full((n_chunks, stride), CANARY, dtype=torch.uint8, device='cuda')
        sizes = torch.full((n_chunks,), -1, dtype=torch.int64, device='cuda')
        _lib.check(lib.vs_deflate_chunks(src.data_ptr(), a.size, chunk, slots.data_ptr(), stride, sizes.data_ptr(), _lib.stream_ptr()), name)
        torch.cuda.synchronize()
        sizes_h, slots_h = sizes.cpu().numpy(), slots.cpu().numpy()
        lens = np.minimum(chunk, a.size - chunk * np.arange(n_chunks))
        assert np.all(sizes_h >= 5) and np.all(sizes_h <= lens + ops.DEFLATE_SLOT_EXTRA), name
        behind = np.arange(stride)[None, :] >= sizes_h[:, None]
        assert np.all(slots_h[behind] == CANARY), name
        stream = b''.join(slots_h[k, :sizes_h[k]].tobytes() for k in range(n_chunks))
        assert _inflate_raw(stream + D.FINAL_BLOCK) == a.tobytes(), name
        if name in ('random_40000', 'all_256'):
            assert np.array_equal(sizes_h, lens + ops.DEFLATE_SLOT_EXTRA), name  # stored: the worst case exactly


@pytest.mark.parametrize('name', ['random_40000', 'fibonacci', 'odd_len_off3'])
@pytest.mark.parametrize('misalign', [0, 3])
def test_guard_bytes_round_every_allocation_stay_intact(name, misalign, monkeypatch):
    a = dict(D.corpus())[name]
    src = _device_source(name, a)
    allocs = guarded_ops(monkeypatch, misalign=misalign)
    packed, _ = ops.deflate_raw(src)
    crc = ops.crc32(src, init=5)
    allocs.check()
    assert len(allocs.guards) >= 4                                          # slots, sizes, packed, the CRC's partials
    assert _inflate_raw(packed.cpu().numpy().tobytes() + D.FINAL_BLOCK) == a.tobytes() and crc == zlib.crc32(a.tobytes(), 5)


def test_crc32_equals_zlib_on_the_corpus_and_on_wider_dtypes():
    for name, a in D.corpus():
        t = _device_source(name, a)
        for init in (0, 0xDEADBEEF):
            assert ops.crc32(t, init) == zlib.crc32(a.tobytes(), init), (name, init)
    wide = np.random.RandomState(3).randint(-2 ** 62, 2 ** 62, size=(7, 3001), dtype=np.int64)
    assert ops.crc32(torch.from_numpy(wide).cuda()) == zlib.crc32(wide.tobytes())
    assert ops.crc32(torch.from_numpy(wide).cuda()[2:5], init=123) == zlib.crc32(wide[2:5].tobytes(), 123)
    half = torch.from_numpy(wide.view(np.float16)[:, :11].copy()).cuda()
    assert ops.crc32(half) == zlib.crc32(half.cpu().numpy().tobytes())


def test_the_devices_own_inflate_reads_what_its_deflate_wrote(compressed):
    picked = [(name, a, packed) for name, (a, packed, _) in compressed.items() if 2 + len(packed) + 2 + 4 <= 1 << 20 and a.size <= 1 << 20]
    assert len(picked) >= len(NAMES) - 2
    streams = [b'\x78\x01' + packed + D.FINAL_BLOCK + zlib.adler32(a.tobytes()).to_bytes(4, 'big') for _, a, packed in picked]
    offsets = np.zeros(len(streams) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in streams], out=offsets[1:])
    out_len = np.array([a.size for _, a, _ in picked], dtype=np.int64)
    out, status, produced = ops.inflate_zlib(torch.from_numpy(np.frombuffer(b''.join(streams), dtype=np.uint8).copy()).cuda(),
                                             torch.from_numpy(offsets).cuda(), torch.from_numpy(out_len).cuda(), max(1, int(out_len.max())))
    status, produced, out = status.cpu().numpy(), produced.cpu().numpy(), out.cpu().numpy()
    for i, (name, a, _) in enumerate(picked):
        assert status[i] == 0 and produced[i] == a.size and np.array_equal(out[i, :a.size], a), (name, ops.INFLATE_STATUS.get(int(status[i])))


def test_size_bars_hold_for_the_kernels_output(compressed):
    def zlib_raw(data, strategy):
        co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, strategy)
        return len(co.compress(data) + co.flush())

    a, packed, _ = compressed['mmnist']
    level6 = zlib_raw(a.tobytes(), zlib.Z_DEFAULT_STRATEGY)
    print('Moving-MNIST set: kernel %d bytes, zlib level 6 %d (ratio %.4f)' % (len(packed) + 2, level6, (len(packed) + 2) / level6))
    assert len(packed) + 2 <= 1.10 * level6
    a, packed, _ = compressed['noisy_probe']
    huffman = zlib_raw(a.tobytes(), zlib.Z_HUFFMAN_ONLY)
    print('noisy probe: kernel %d bytes, zlib Z_HUFFMAN_ONLY %d (ratio %.4f)' % (len(packed) + 2, huffman, (len(packed) + 2) / huffman))
    assert len(packed) + 2 <= 1.10 * huffman


def test_slabs_give_the_same_bytes_as_one_pass():
    a = np.concatenate([dict(D.corpus())['mmnist'][:9 * D.L], dict(D.corpus())['random_40000'][:D.L - 77]])
    assert -(-a.size // D.L) == 10
    t = torch.from_numpy(a.copy()).cuda()
    whole, n_whole = ops.deflate_raw(t)
    pieces = list(ops.deflate_raw_slabs(t, slab_bytes=3 * D.L))
    assert [n for _, n in pieces] == [3, 3, 3, 1] and n_whole == 10
    joined = b''.join(p.cpu().numpy().tobytes() for p, _ in pieces)
    assert joined == whole.cpu().numpy().tobytes()
    cat, n_cat = ops.deflate_raw(t, slab_bytes=3 * D.L)
    assert n_cat == 10 and cat.cpu().numpy().tobytes() == joined
    assert _inflate_raw(joined + D.FINAL_BLOCK) == a.tobytes()
    crc = 0
    for lo in range(0, a.size, 3 * D.L):                                    # the CRC continued slab by slab equals the CRC of the whole
        crc = ops.crc32(t[lo:lo + 3 * D.L], init=crc)
    assert crc == ops.crc32(t) == zlib.crc32(a.tobytes())


def test_cli_with_the_device_compressor_writes_the_reference_arrays(tmp_path, monkeypatch):
    from spatiotemporal_variable_separation_amd.data import moving_mnist
    c = MI.CASES['default']
    images, labels = MI.standins('default')
    want = MI.golden('default')
    files = {}
    for mode in ('device', 'host'):
        data = MI.write_t10k(str(tmp_path / mode), images, labels)
        monkeypatch.setenv(make_test_set.COMPRESS_ENV, mode)
        make_test_set.main(['--data_dir', data, '--seq_len', str(c['seq_len']), '--device', '0'])
        files[mode] = os.path.join(data, 'mmnist_test_2digits_64.npz')
        with np.load(files[mode]) as z:
            assert z.files == list(MI.ARRAYS)
            for k in MI.ARRAYS:
                assert z[k].dtype == want[k].dtype and z[k].shape == want[k].shape and np.array_equal(z[k], want[k]), (mode, k)
    import zipfile
    with zipfile.ZipFile(files['device']) as zd, zipfile.ZipFile(files['host']) as zh:
        assert zd.testzip() is None and zd.namelist() == zh.namelist()
        assert [(i.file_size, i.CRC) for i in zd.infolist()] == [(i.file_size, i.CRC) for i in zh.infolist()]
    try:
        sets = [moving_mnist.MovingMNIST.make_dataset(os.path.dirname(files[mode]), 64, 3, 13, 4, True, 2, False, device='cuda')
                for mode in ('device', 'host')]
        assert len(sets[0]) == len(sets[1]) == 12 and torch.equal(sets[0].data, sets[1].data)
    finally:
        moving_mnist.forget_generated()


def test_generate_device_returns_the_files_arrays_on_the_device(tmp_path):
    c = MI.CASES['default']
    images, labels = MI.standins('default')
    want = MI.golden('default')
    data = MI.write_t10k(str(tmp_path / 'data'), images, labels)
    got = make_test_set.generate_device(data, c['seq_len'], c['seed'], c['digits'], c['frame'], c['speed'], torch.device('cuda', 0))
    assert list(got) == list(MI.ARRAYS)
    for k in MI.ARRAYS:
        assert got[k].is_cuda and got[k].is_contiguous()
        h = got[k].cpu().numpy()
        assert h.dtype == want[k].dtype and h.shape == want[k].shape and np.array_equal(h, want[k]), k
    with pytest.raises(_lib.VarsepHipError, match='device tensors'):
        make_test_set.save_test_set(str(tmp_path / 'x.npz'), {k: v.cpu().numpy() for k, v in got.items()}, compress='device')

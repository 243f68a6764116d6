"""GPU: vs_deflate_chunks_window (csrc/vs_deflate.hip) through ops.deflate_raw(match='window') -- byte for byte the host build of the same
logic (csrc/vs_deflate_window_core.h) on the corpus, the inputs of tests/deflate_window_inputs.py and 60 mixtures, at three chunk lengths
and from source pointers 1 and 3 bytes off their allocation; the history across slab borders; guard bytes round slots, sizes and every
allocation; and the .npz route with match='window'."""
import os
import zipfile
import zlib

import numpy as np
import pytest
import torch

import deflate_inputs as D
import deflate_window_inputs as WI
from guard_util import CANARY, guarded_ops
from spatiotemporal_variable_separation_amd import _lib, ops
from spatiotemporal_variable_separation_amd.utils import savez

pytestmark = pytest.mark.gpu

L = D.L


def _device_source(a, off=0):
    """The input on the device, starting `off` bytes into its allocation."""
    buf = torch.empty(a.size + off, dtype=torch.uint8, device='cuda')
    buf[off:] = torch.from_numpy(a.copy())
    t = buf[off:]
    assert t.data_ptr() % 4 == off % 4 and t.is_contiguous()
    return t


def _inflate_raw(stream):
    d = zlib.decompressobj(-15)
    out = d.decompress(stream)
    assert d.eof and not d.unused_data
    return out


def _cases():
    """[(name, array, bytes between the allocation and the source pointer)]: the corpus, the new inputs (those with a history as whole
    arrays: the kernel's own chunks see the history the host's do) and 60 mixtures."""
    out = [(name, a, D.SOURCE_OFFSET.get(name, 0)) for name, a in D.corpus()]
    out += [(name, a, 0) for name, a, _ in WI.inputs()]
    out += [('mixture %d' % k, a, (0, 1, 3)[k % 3]) for k, a in enumerate(D.mixtures(500)[:60])]
    return out


@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('deflate_window_gpu')
    exe, _ = WI.compile_host_check(tmp)
    return exe, tmp


def test_kernel_bytes_equal_the_host_builds_at_the_default_chunk(host_exe):
    exe, tmp = host_exe
    cases = _cases()
    records, stdout = WI.run_host_check(exe, [(a, 0) for _, a, _ in cases], tmp)
    assert stdout.strip().splitlines()[-1].endswith('mismatches 0'), stdout[-2000:]
    window_chunks = 0
    for (name, a, off), rec in zip(cases, records):
        packed, n_chunks = ops.deflate_raw(_device_source(a, off), match='window')
        assert packed.dtype == torch.uint8 and packed.is_cuda and packed.dim() == 1
        got = packed.cpu().numpy().tobytes()
        assert n_chunks == rec['n_chunks'] and len(got) == len(rec['stream']) and got == rec['stream'], name
        window_chunks += sum(1 for f in rec['forms'] if f >= 4)
    assert window_chunks > 100                                              # the window parse was written, not only the runs parse kept
    a = dict((n, a) for n, a, _ in cases)['mmnist_video_major']
    got, _ = ops.deflate_raw(_device_source(a), match='window')
    runs, _ = ops.deflate_raw(_device_source(a))
    assert _inflate_raw(got.cpu().numpy().tobytes() + D.FINAL_BLOCK) == a.tobytes()
    print('video-major Moving-MNIST: window %d bytes, runs %d' % (got.numel() + 2, runs.numel() + 2))
    assert got.numel() + 2 <= 0.5 * (runs.numel() + 2)


@pytest.mark.parametrize('chunk', [1024, 4096])
def test_kernel_bytes_equal_the_host_builds_at_small_chunks(host_exe, chunk):
    exe, tmp = host_exe
    picked = [(n, a, off) for n, a, off in _cases() if a.size <= 3 * L + 5 and not n.startswith('mixture')] + \
             [(n, a, off) for n, a, off in _cases() if n.startswith('mixture')][:20]
    assert {off for _, _, off in picked} == {0, 1, 3} and len(picked) > 40
    records, stdout = WI.run_host_check(exe, [(a, 0) for _, a, _ in picked], tmp, chunk=chunk, tag='chunk%d' % chunk)
    assert stdout.strip().splitlines()[-1].endswith('mismatches 0'), stdout[-2000:]
    for (name, a, off), rec in zip(picked, records):
        packed, n_chunks = ops.deflate_raw(_device_source(a, off), chunk_bytes=chunk, match='window')
        assert n_chunks == rec['n_chunks'] == -(-a.size // chunk) and packed.cpu().numpy().tobytes() == rec['stream'], name


def test_the_entry_point_with_a_history_before_the_source_pointer(host_exe):
    """Compressing from an offset with history_bytes = the offset (1, 100, 4096) and from a chunk border with 32768, through the entry
    point itself with the tightest slots and one workgroup's workspace: the host's bytes, and guard bytes behind every slot and sizes."""
    exe, tmp = host_exe
    lib = _lib.load_library()
    cases = [(a, h) for _, a, h in WI.inputs() if h] + [(dict((n, a) for n, a, _ in WI.inputs())['history_cut'][L:], L)]
    records, _ = WI.run_host_check(exe, cases, tmp, tag='history')
    for (a, h), rec in zip(cases, records):
        src = _device_source(a, 3)
        n = a.size - h
        n_chunks, stride = -(-n // L), L + ops.DEFLATE_SLOT_EXTRA
        slots = torch.full((n_chunks * stride + 64,), CANARY, dtype=torch.uint8, device='cuda')
        sizes = torch.full((n_chunks + 8,), -1, dtype=torch.int64, device='cuda')
        work = torch.full((ops.DEFLATE_WINDOW_GROUP_BYTES // 4 + 16,), -1, dtype=torch.int32, device='cuda')
        _lib.check(lib.vs_deflate_chunks_window(src.data_ptr() + h, h, n, L, slots.data_ptr(), stride, sizes.data_ptr(), work.data_ptr(),
                                                ops.DEFLATE_WINDOW_GROUP_BYTES, _lib.stream_ptr()), 'vs_deflate_chunks_window')
        torch.cuda.synchronize()
        sizes_h, slots_h, work_h = sizes.cpu().numpy(), slots.cpu().numpy(), work.cpu().numpy()
        assert sizes_h[:n_chunks].tolist() == rec['sizes'] and np.all(sizes_h[n_chunks:] == -1), h
        assert np.all(work_h[ops.DEFLATE_WINDOW_GROUP_BYTES // 4:] == -1), h
        rows = slots_h[:n_chunks * stride].reshape(n_chunks, stride)
        assert np.all(rows[np.arange(stride)[None, :] >= sizes_h[:n_chunks, None]] == CANARY) and np.all(slots_h[n_chunks * stride:] == CANARY), h
        assert b''.join(rows[k, :sizes_h[k]].tobytes() for k in range(n_chunks)) == rec['stream'], h


def test_slabs_see_the_history_across_their_borders():
    a = dict((n, a) for n, a, _ in WI.inputs())['mmnist_video_major'][:9 * L + 777]
    t = _device_source(a)
    whole, n_whole = ops.deflate_raw(t, match='window')
    pieces = list(ops.deflate_raw_slabs(t, slab_bytes=2 * L, match='window'))
    assert [n for _, n in pieces] == [2, 2, 2, 2, 2] and n_whole == 10
    joined = b''.join(p.cpu().numpy().tobytes() for p, _ in pieces)
    assert joined == whole.cpu().numpy().tobytes() and _inflate_raw(joined + D.FINAL_BLOCK) == a.tobytes()
    cat, n_cat = ops.deflate_raw(t, slab_bytes=2 * L, match='window')
    assert n_cat == 10 and cat.cpu().numpy().tobytes() == joined
    alone = b''.join(ops.deflate_raw(t[lo:lo + 2 * L].clone(), match='window')[0].cpu().numpy().tobytes() for lo in range(0, a.size, 2 * L))
    assert _inflate_raw(alone + D.FINAL_BLOCK) == a.tobytes() and len(alone) > len(joined)   # slabs that do not see what lies before them


@pytest.mark.parametrize('name', ['random_40000', 'stride_4097', 'fibonacci_distances'])
@pytest.mark.parametrize('misalign', [0, 3])
def test_guard_bytes_round_every_allocation_stay_intact(name, misalign, monkeypatch):
    a = dict([(n, a) for n, a in D.corpus()] + [(n, a) for n, a, _ in WI.inputs()])[name]
    src = _device_source(a, 1)
    allocs = guarded_ops(monkeypatch, misalign=misalign)
    packed, _ = ops.deflate_raw(src, match='window')
    allocs.check()
    assert len(allocs.guards) >= 4                                          # slots, sizes, the workspace, packed
    assert _inflate_raw(packed.cpu().numpy().tobytes() + D.FINAL_BLOCK) == a.tobytes()


def test_npz_files_with_the_window_matcher_read_back_and_are_smaller(tmp_path, monkeypatch):
    rs = np.random.RandomState(77)
    digits = (rs.rand(6, 1, 64, 64, 1) < 0.08).astype(np.uint8) * rs.randint(1, 256, size=(6, 1, 64, 64, 1)).astype(np.uint8)
    mnist = np.ascontiguousarray(np.stack([np.roll(digits[:, 0], 2 * t, axis=2) for t in range(10)], axis=1))      # [6, 10, 64, 64, 1]
    base = rs.randint(0, 256, size=(4, 1, 64, 64, 3)).astype(np.uint8)
    chairs = np.ascontiguousarray(np.stack([np.roll(base[:, 0], t, axis=1) for t in range(5)], axis=1))              # [4, 5, 64, 64, 3]
    assert mnist.shape == (6, 10, 64, 64, 1) and chairs.shape == (4, 5, 64, 64, 3)
    arrays = dict(mnist=torch.from_numpy(mnist).cuda(), chairs=torch.from_numpy(chairs).cuda(), floats=np.arange(7, dtype=np.float32))
    monkeypatch.delenv(savez.MATCH_ENV, raising=False)
    paths = {k: str(tmp_path / (k + '.npz')) for k in ('window', 'runs', 'default', 'env')}
    savez.savez_compressed(paths['window'], arrays, compress='device', match='window')
    savez.savez_compressed(paths['runs'], arrays, compress='device', match='runs')
    savez.savez_compressed(paths['default'], arrays, compress='device')
    monkeypatch.setenv(savez.MATCH_ENV, 'window')
    savez.savez_compressed(paths['env'], arrays, compress='device')
    blobs = {k: open(p, 'rb').read() for k, p in paths.items()}
    assert blobs['default'] == blobs['runs'] and blobs['env'] == blobs['window']   # nothing said: the file of the time before the matcher
    for k in ('window', 'runs'):
        with np.load(paths[k]) as z:
            assert z.files == list(arrays)
            assert np.array_equal(z['mnist'], mnist) and np.array_equal(z['chairs'], chairs) and np.array_equal(z['floats'], arrays['floats'])
        with zipfile.ZipFile(paths[k]) as z:
            assert z.testzip() is None
    with zipfile.ZipFile(paths['window']) as zw, zipfile.ZipFile(paths['runs']) as zr:
        sizes = {i.filename: (i.compress_size, j.compress_size) for i, j in zip(zw.infolist(), zr.infolist())}
    print('compressed bytes (window, runs):', sizes)
    assert sizes['mnist.npy'][0] < sizes['mnist.npy'][1] and sizes['chairs.npy'][0] < sizes['chairs.npy'][1]
    assert os.path.getsize(paths['window']) < os.path.getsize(paths['runs'])

"""PNG encoding on the device (csrc/vs_png_encode.hip) on an MI355X: vs_png_filter against tests/png_inputs.py's `filter_rows` /
`adaptive_ftypes`, vs_deflate_streams against zlib's inflate and against the single-array encoder on every stream alone, whole files
from ops.png_encode_u8 against the host build of the same logic, zlib, the tree's own readers and its own device decoder, and
`gen_chairs.generate` with the device encoder against the host route.  Everything is byte equality."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import deflate_window_inputs as DW
import guard_util as G
import png_encode_inputs as E
import png_inputs as P
import resample_inputs as I
from spatiotemporal_variable_separation_amd import ops
from spatiotemporal_variable_separation_amd.data import chairs as C
from spatiotemporal_variable_separation_amd.preprocessing.chairs import gen_chairs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCHERS = ('runs', 'window')


def _filter(imgs, mode, **kw):
    raw = ops.png_filter(torch.from_numpy(np.ascontiguousarray(imgs)).to(DEV), mode, **kw)
    torch.cuda.synchronize()
    return raw.cpu().numpy()


# ---- the filters -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', E.FILTER_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_filter_every_mode_equals_the_reference(shape):
    """Three DIFFERENT images per launch: a kernel that takes the previous image's last row for the row above row 0 fails on image 1."""
    imgs = E.images(3, shape)
    assert len({img.tobytes() for img in imgs}) >= 2
    for mode in range(6):
        got, want = _filter(imgs, mode), E.filtered(imgs, mode)
        for i in range(3):
            assert got[i].tobytes() == want[i], (shape, mode, i)
    assert ops.png_filter(torch.from_numpy(imgs).to(DEV), 'paeth').cpu().numpy().tobytes() == b''.join(E.filtered(imgs, 4))


def test_filter_ties_go_to_the_lowest_type_and_residuals_count_signed():
    for name, imgs in E.special_images().items():
        got, want = _filter(imgs, 'adaptive'), E.filtered(imgs, E.ADAPTIVE)
        for i in range(len(imgs)):
            assert got[i].tobytes() == want[i], (name, i)
    zero = _filter(E.special_images()['zero'], 'adaptive').reshape(3, 6, -1)
    assert (zero[:, :, 0] == 0).all()                                      # five sums of 0: type 0
    stripes = E.special_images()['stripes']
    unsigned = [int(np.argmin([np.frombuffer(P.filter_rows(stripes[1], [f] * 6), np.uint8).reshape(6, -1)[y, 1:].astype(np.int64).sum()
                               for f in range(5)])) for y in range(6)]
    assert unsigned != P.adaptive_ftypes(stripes[1])                       # the case tells the signed reading from the unsigned one


def test_filter_reads_pixels_at_an_odd_address_and_keeps_to_its_rows_of_raw():
    h, w, c = 5, 22, 3
    imgs = E.images(3, (h, w, c), seed=9)
    S = h * (1 + w * c)
    buf = torch.zeros(3 + imgs.size, dtype=torch.uint8, device=DEV)
    for lead in (1, 3):
        view = buf[lead:lead + imgs.size].view(imgs.shape)
        view.copy_(torch.from_numpy(imgs))
        assert view.data_ptr() % 2 == 1 and view.is_contiguous()
        out, guard = G.window((3, S), torch.uint8, ld=S + 37, offset=lead, device=DEV)
        got = ops.png_filter(view, 'adaptive', out=out)
        assert got.data_ptr() == out.data_ptr() and out.stride(0) == S + 37
        guard.check()                                                      # the 37 bytes behind every image and the bands are untouched
        want = E.filtered(imgs, E.ADAPTIVE)
        for i in range(3):
            assert out[i].cpu().numpy().tobytes() == want[i], (lead, i)


# ---- the streams -----------------------------------------------------------------------------------------------------------------
def _stream_content(n):
    base = np.concatenate([DW.periods(), DW.one_distance_symbol()])
    assert base.size >= n
    return base[:n]


@pytest.mark.parametrize('match', MATCHERS)
@pytest.mark.parametrize('stream_bytes,chunk', [(1, 1024), (1023, 1024), (1024, 1024), (1025, 1024), (2561, 1024), (2561, None)])
def test_streams_are_independent_and_equal_the_single_array_encoder(stream_bytes, chunk, match):
    """Stream s + 1 is a byte copy of stream s, 37 bytes of junk apart: a match across a stream border would be the cheapest parse."""
    n, stride = 4, stream_bytes + 37
    one = _stream_content(stream_bytes)
    host = np.random.RandomState(77).randint(0, 256, size=(n, stride)).astype(np.uint8)
    host[:, :stream_bytes] = one
    raw = torch.from_numpy(host).to(DEV)
    K = -(-stream_bytes // (chunk or E.DEFAULT_CHUNK))
    slots, sizes = ops.deflate_streams(raw, stream_bytes, chunk, match)
    assert tuple(sizes.shape) == (n * K,) and slots.shape[0] == n * K
    slots_h, sizes_h = slots.cpu().numpy(), sizes.cpu().numpy()
    alone, n_chunks = ops.deflate_raw(torch.from_numpy(one.copy()).to(DEV), chunk, match=match)
    alone = alone.cpu().numpy().tobytes()
    assert n_chunks == K
    for s in range(n):
        stream = b''.join(slots_h[s * K + k, :sizes_h[s * K + k]].tobytes() for k in range(K))
        assert all(5 <= sizes_h[s * K + k] <= min(chunk or E.DEFAULT_CHUNK, stream_bytes - k * (chunk or E.DEFAULT_CHUNK)) + E.SLOT_EXTRA for k in range(K))
        inflater = zlib.decompressobj(-15)                                 # a fresh decoder per stream: it has seen no other stream
        assert inflater.decompress(stream + b'\x03\x00') == one.tobytes() and inflater.eof, (s, stream_bytes, match)
        assert stream == alone, (s, stream_bytes, match)                   # the existing encoder on this stream alone, byte for byte
        assert all(d <= p for p, _, d in DW.matches(stream + b'\x03\x00')), s
    if match == 'window':                                                  # the workspace size changes no byte
        for groups in (1, 3):
            slots2, sizes2 = ops.deflate_streams(raw, stream_bytes, chunk, match, groups=groups)
            assert torch.equal(sizes2, sizes)
            s2 = slots2.cpu().numpy()
            assert all(np.array_equal(s2[c, :sizes_h[c]], slots_h[c, :sizes_h[c]]) for c in range(n * K)), groups


# ---- whole files -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_files(tmp_path_factory):
    """{(n, shape, chunk, match): (rows, files)} of the host build of the same logic, for every case of E.ENCODE_CASES: computed once."""
    tmp = tmp_path_factory.mktemp('png_encode_host')
    exe, _ = E.compile_host_check(tmp)
    keys = [(n, shape, chunk, match) for n, shape, chunk in E.ENCODE_CASES for match in MATCHERS]
    cases = [(E.images(n, shape, seed=n), E.ADAPTIVE, chunk or E.DEFAULT_CHUNK, match) for n, shape, chunk, match in keys]
    records, _ = E.run_host_check(exe, cases, tmp)
    return dict(zip(keys, records))


@pytest.mark.parametrize('n,shape,chunk', E.ENCODE_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_encode_equals_the_host_build_and_every_reader_returns_the_pixels(n, shape, chunk, host_files, tmp_path):
    imgs = E.images(n, shape, seed=n)
    h, w, c = shape
    S = h * (1 + w * c)
    K = -(-S // (chunk or E.DEFAULT_CHUNK))
    want_rows = E.filtered(imgs, E.ADAPTIVE)
    made = {}
    for match in MATCHERS:
        files, sizes = ops.png_encode_u8(torch.from_numpy(imgs).to(DEV), match=match, chunk_bytes=chunk)
        assert files.is_cuda and files.dtype == torch.uint8 and sizes.dtype == torch.int64 and tuple(sizes.shape) == (n,)
        files_h, sizes_h = files.cpu().numpy(), sizes.cpu().numpy()
        blobs = [files_h[i, :sizes_h[i]].tobytes() for i in range(n)]
        rows, host = host_files[(n, shape, chunk, match)]
        for i in range(n):
            assert rows[i] == want_rows[i]
            assert blobs[i] == host[i], (match, i, len(blobs[i]), len(host[i]))                  # the kernels' bytes are the host's bytes
            E.check_file(blobs[i], imgs[i], want_rows[i], '%s image %d' % (match, i))
            assert sizes_h[i] <= E.FIXED_BYTES + S + E.SLOT_EXTRA * K
        made[match] = blobs
    assert all(len(a) <= len(b) for a, b in zip(made['window'], made['runs']))                  # per chunk never larger, so per file
    if c == 3:
        image_module = C._pil_image()
        for i, blob in enumerate(made['window']):
            path = str(tmp_path / ('%d.png' % i))
            with open(path, 'wb') as f:
                f.write(blob)
            assert np.array_equal(C.read_png_rgb8(path), imgs[i])
            if image_module is not None:
                assert np.array_equal(np.asarray(image_module.open(path).convert('RGB')), imgs[i])
        for match in MATCHERS:                                             # the tree's own decoder reads the tree's own encoder
            pixels, status = ops.png_decode_rgb8(made[match], device=DEV)
            assert status.cpu().tolist() == [0] * n and np.array_equal(pixels.cpu().numpy(), imgs), match


@pytest.mark.parametrize('misalign', [0, 1])
def test_no_launch_writes_outside_its_outputs(monkeypatch, misalign):
    """Guard bands round raw, slots, sizes, files and file sizes; misalign=1 puts each one element off its allocation."""
    allocs = G.guarded_ops(monkeypatch, misalign=misalign)
    imgs = E.images(5, (37, 53, 3), seed=5)
    files, sizes = ops.png_encode_u8(torch.from_numpy(imgs).to(DEV), chunk_bytes=1024)
    assert len(allocs.guards) >= 5 and files.data_ptr() % 2 == misalign
    allocs.check()
    files_h, sizes_h = files.cpu().numpy(), sizes.cpu().numpy()
    for i in range(5):
        assert (files_h[i, sizes_h[i]:] == G.CANARY).all(), i              # bytes of a file's row beyond the file stay untouched
        E.check_file(files_h[i, :sizes_h[i]].tobytes(), imgs[i], E.filtered(imgs[i:i + 1], E.ADAPTIVE)[0])
    # sizes that are none: the image is flagged, its row is not written, its neighbours are
    raw = ops.png_filter(torch.from_numpy(imgs).to(DEV))
    slots, chunk_sizes = ops.deflate_streams(raw, raw.shape[1], 1024, 'runs')
    K = chunk_sizes.numel() // 5
    chunk_sizes[1 * K + 2] = slots.shape[1] + 1
    chunk_sizes[3 * K] = -1
    files2, sizes2 = ops.png_assemble(raw, slots, chunk_sizes, 37, 53, 3)
    allocs.check()
    assert [int(v) >= 0 for v in sizes2.cpu()] == [True, False, True, False, True]
    f2 = files2.cpu().numpy()
    assert (f2[1] == G.CANARY).all() and (f2[3] == G.CANARY).all()


# ---- gen_chairs --------------------------------------------------------------------------------------------------------------------
class _ThreeViews(C.Chairs):
    max_length = 3                                                         # the trees of this test hold three views per object


def test_generate_with_the_device_encoder_against_the_host_route(tmp_path):
    trees = {d: I.write_raw_tree(tmp_path / d, 2, 3) for d in ('host', 'device')}
    timings = {}
    assert gen_chairs.generate(trees['host'], 64, torch.device(DEV), box=I.RAW_BOX, encode='host') == 6
    assert gen_chairs.generate(trees['device'], 64, torch.device(DEV), box=I.RAW_BOX, encode='device', timings=timings) == 6
    assert {'encode', 'download', 'write'} <= set(timings) and timings['encode'] > 0
    _same_trees(trees, 2, 3)
    for train in (True, False):
        sets = [_ThreeViews(train, trees[d], 1, seq_len=3, device=DEV) for d in ('host', 'device')]
        first = [s.batch(list(range(min(len(s), 4)))) for s in sets]
        assert torch.equal(first[0][0], first[1][0]) and torch.equal(first[0][1], first[1][1])


def _same_trees(trees, n_objects, n_views):
    """Both routes wrote the same file names, every pair of files decodes to the same pixels, and the device's files are sound."""
    listing = {d: sorted(os.path.relpath(os.path.join(p, f), tree) for p, _, fs in os.walk(tree) for f in fs) for d, tree in trees.items()}
    assert listing['host'] == listing['device'] and len(listing['host']) == 1 + n_objects * 2 * n_views
    for name in I.raw_object_names(n_objects):
        for i in range(n_views):
            paths = {d: os.path.join(tree, 'rendered_chairs', name, 'renders', '%d.png' % i) for d, tree in trees.items()}
            want = C.read_png_rgb8(paths['host'])
            assert want.shape == (64, 64, 3) and np.array_equal(C.read_png_rgb8(paths['device']), want)
            E.check_file(open(paths['device'], 'rb').read(), want, E.filtered(want[None], E.ADAPTIVE)[0], paths['device'])


def test_main_in_a_fresh_process_takes_the_encoder_from_the_environment(tmp_path):
    """`main` has the crop box of the original renders, so these two trees hold 600 x 600 ones (one object, three views)."""
    trees = {d: I.write_raw_tree(tmp_path / d, 1, 3, size=600) for d in ('host', 'device')}
    assert gen_chairs.generate(trees['host'], 64, torch.device(DEV), encode='host') == 3
    env = dict(os.environ, **{C.ENCODE_ENV: 'device'})
    r = subprocess.run([sys.executable, '-m', 'spatiotemporal_variable_separation_amd.preprocessing.chairs.gen_chairs', '--data_dir', trees['device'],
                        '--device', '0'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'wrote 3 images' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    _same_trees(trees, 1, 3)
    blob = open(os.path.join(trees['device'], 'rendered_chairs', I.raw_object_names(1)[0], 'renders', '0.png'), 'rb').read()
    image_module = C._pil_image()
    if image_module is not None:                                           # PIL's `save` writes other bytes: the device route ran in the child
        assert blob != open(os.path.join(trees['host'], 'rendered_chairs', I.raw_object_names(1)[0], 'renders', '0.png'), 'rb').read()

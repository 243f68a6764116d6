"""PNG decoding on the device (csrc/vs_png.hip) on an MI355X: vs_inflate_zlib against `zlib.decompress`, vs_png_unfilter against the
source images, the status of every kind of damaged stream, whole PNG files and the three raw-render routes against the host decoder,
and guard bytes round every output.  Everything is byte equality."""
import os
import zlib

import numpy as np
import pytest
import torch

import guard_util as G
import png_inputs as P
import resample_inputs as I
from spatiotemporal_variable_separation_amd import ops
from spatiotemporal_variable_separation_amd.data import chairs as C
from spatiotemporal_variable_separation_amd.preprocessing.chairs import gen_chairs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _pack(streams, lead=1):
    """(packed uint8 on the device, starting `lead` bytes into its allocation, offsets int64 [n + 1]) of streams laid back to back."""
    offsets = np.zeros(len(streams) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in streams], out=offsets[1:])
    buf = torch.from_numpy(np.frombuffer(bytearray(bytes(lead) + b''.join(streams) + b'\0'), dtype=np.uint8).copy()).to(DEV)
    return buf[lead:lead + int(offsets[-1])], torch.from_numpy(offsets).to(DEV)


def _inflate(streams, lengths, stride=None, lead=1):
    packed, offsets = _pack(streams, lead)
    stride = max(max(lengths), 1) if stride is None else stride
    out, status, produced = ops.inflate_zlib(packed, offsets, torch.tensor(lengths, dtype=torch.int64, device=DEV), stride)
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy(), produced.cpu().numpy()


@pytest.fixture(scope='module')
def corpus():
    return P.corpus()


def test_inflate_corpus_equals_zlib(corpus):
    streams = [s for _, s, _ in corpus]
    lengths = [len(zlib.decompress(s)) for s in streams]
    assert any(int(o) % 2 for o in np.cumsum([len(s) for s in streams]))   # odd offsets inside the packed buffer, itself at an odd address
    out, status, produced = _inflate(streams, lengths)
    for i, (name, s, _) in enumerate(corpus):
        assert status[i] == 0, (name, int(status[i]), int(produced[i]))
        assert produced[i] == lengths[i], name
        assert out[i, :lengths[i]].tobytes() == zlib.decompress(s), name


@pytest.fixture(scope='module')
def payload(corpus):
    h, w = P.PNG_SIZE
    return P.filter_rows(P.sample_image(h, w, seed=3), [y % 5 for y in range(h)])


def test_every_damage_has_its_status_and_the_neighbours_decode(payload):
    damaged = P.damaged_streams(payload)
    good = P.deflate(payload, 6)
    streams, want = [good], [P.OK]
    for name, (s, st) in damaged.items():
        streams += [s, good]
        want += [st, P.OK]
    out, status, produced = _inflate(streams, [len(payload)] * len(streams))
    assert list(status) == want, dict(zip(['good'] + [n for name in damaged for n in (name, 'good')], status))
    for i, st in enumerate(want):
        if st == P.OK:
            assert out[i].tobytes() == payload and produced[i] == len(payload)
        else:
            assert 0 <= produced[i] <= len(payload)
    assert set(want) >= {P.INPUT, P.ADLER, P.BLOCK_TYPE, P.DISTANCE, P.HEADER, P.OUT_LONG, P.OUT_SHORT}


def test_damaged_files_through_png_decode_rgb8(payload):
    h, w = P.PNG_SIZE
    img = P.sample_image(h, w, seed=3)
    good = P.png_from_stream(w, h, P.deflate(payload, 6))
    damaged = dict(P.damaged_streams(payload))
    bad_filter = bytearray(payload)
    bad_filter[5 * (1 + 3 * w)] = 7                                        # the filter byte of row 5
    damaged['filter_7'] = (P.deflate(bytes(bad_filter), 6), P.BAD_FILTER)
    names = ['good0'] + [n for name in damaged for n in (name + '.png', 'after_' + name)]
    blobs = [good] + [b for s, _ in damaged.values() for b in (P.png_from_stream(w, h, s), good)]
    pixels, status = ops.png_decode_rgb8(blobs, names, DEV)
    status, pixels = status.cpu().numpy(), pixels.cpu().numpy()
    want = [P.OK] + [s for _, st in damaged.values() for s in (st, P.OK)]
    assert list(status) == want
    for i, st in enumerate(want):
        if st == P.OK:
            assert np.array_equal(pixels[i], img), names[i]
    for name, (s, st) in damaged.items():                                  # the first failed file is named with its reason
        with pytest.raises(ValueError, match=r'%s\.png: %s' % (name, ops.INFLATE_STATUS[st][:20])):
            ops.png_decode_rgb8([good, P.png_from_stream(w, h, s), good], ['a', name + '.png', 'c'], DEV, check_status=True)


def _unfilter(imgs, ftypes_of, stride_extra=0):
    n, h, w, c = imgs.shape
    size = h * (1 + w * c)
    raw = np.full((n, size + stride_extra), 0xEE, dtype=np.uint8)
    for i in range(n):
        raw[i, :size] = np.frombuffer(P.filter_rows(imgs[i], ftypes_of(i, h)), dtype=np.uint8)
    status = torch.zeros(n, dtype=torch.int32, device=DEV)
    out = ops.png_unfilter(torch.from_numpy(raw).to(DEV), status, h, w, c)
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize('c', [3, 4])
@pytest.mark.parametrize('h,w', [(1, 1), (1, 5), (7, 13), (64, 64), (65, 3), (130, 9)])
def test_unfilter_every_type_on_all_rows_and_cycling(h, w, c):
    # images 0..4: type i on all rows (the first row included); image 5: type y % 5; image 6: type (y + 3) % 5
    imgs = np.stack([P.sample_image(h, w, c, seed=i) for i in range(7)])
    out, status = _unfilter(imgs, lambda i, rows: [i] * rows if i < 5 else [(y + 3 * (i - 5)) % 5 for y in range(rows)], stride_extra=3)
    assert not status.any()
    for i in range(7):
        assert np.array_equal(out[i], imgs[i]), (i, int((out[i] != imgs[i]).sum()))


def test_unfilter_600_x_600_mixed_filters_and_skipped_images():
    rng = np.random.RandomState(P.SEED)
    imgs = np.stack([P.sample_image(600, 600, 3, seed=20), rng.randint(0, 256, size=(600, 600, 3)).astype(np.uint8)])
    types = [P.adaptive_ftypes(imgs[0]), [int(t) for t in rng.randint(0, 5, size=600)]]
    assert len(set(types[0])) >= 3
    out, status = _unfilter(imgs, lambda i, rows: types[i])
    assert not status.any() and np.array_equal(out, imgs)
    # an image that failed in the inflate launch is skipped and keeps its status; a filter byte above 4 marks only its own image
    small = np.stack([P.sample_image(9, 6, 3, seed=i) for i in range(3)])
    raw = np.stack([np.frombuffer(P.filter_rows(small[i], [4] * 9), dtype=np.uint8) for i in range(3)]).copy()
    raw[2, 3 * 19] = 5
    status = torch.tensor([0, P.ADLER, 0], dtype=torch.int32, device=DEV)
    out = ops.png_unfilter(torch.from_numpy(raw).to(DEV), status, 9, 6, 3)
    assert status.cpu().tolist() == [0, P.ADLER, P.BAD_FILTER] and np.array_equal(out[0].cpu().numpy(), small[0])


def test_png_cases_in_one_batch_and_idat_splits():
    cases = P.png_cases()
    blobs = [P.png_bytes(img, **kw) for img, kw in cases.values()]
    pixels, status = ops.png_decode_rgb8(blobs, list(cases), DEV, check_status=True)
    assert pixels.dtype == torch.uint8 and tuple(pixels.shape) == (len(blobs),) + P.PNG_SIZE + (3,) and pixels.device.type == 'cuda'
    for i, (name, (img, _)) in enumerate(cases.items()):
        assert np.array_equal(pixels[i].cpu().numpy(), img), name
    img = P.sample_image(37, 53, seed=11)
    one, three = (P.png_bytes(img, ftypes='adaptive', n_idat=k) for k in (1, 3))
    assert three.count(b'IDAT') == 3 and one != three
    a, b = ops.png_decode_rgb8([one, three], device=DEV)[0].cpu().numpy()
    assert np.array_equal(a, img) and np.array_equal(b, img)


@pytest.fixture(scope='module')
def raw_tree(tmp_path_factory):
    return I.write_raw_tree(tmp_path_factory.mktemp('png_raw'), 7, 62)


def _paths(tree, k, n_views):
    d = os.path.join(tree, 'rendered_chairs', I.raw_object_names(k + 1)[k], 'renders')
    return [os.path.join(d, f) for f in I.raw_file_names(n_views)]


def test_prepare_renders_device_equals_host(raw_tree):
    paths = _paths(raw_tree, 0, 62) + _paths(raw_tree, 1, 9)
    timings = {}
    got = C.prepare_renders(paths, I.RAW_BOX, 64, torch.device(DEV), C._pil_image(), timings, decode='device')
    want = C.prepare_renders(paths, I.RAW_BOX, 64, torch.device(DEV), C._pil_image(), None, decode='host')
    assert got.device.type == 'cuda' and torch.equal(got, want)
    assert set(timings) == {'decode', 'upload', 'kernel'} and all(v > 0 for v in timings.values())


def test_from_raw_device_equals_host(raw_tree):
    dev = C.Chairs.from_raw(False, raw_tree, 2, seq_len=4, box=I.RAW_BOX, device=DEV, decode='device')
    host = C.Chairs.from_raw(False, raw_tree, 2, seq_len=4, box=I.RAW_BOX, device=DEV, decode='host')
    assert dev.raw_decode == 'device' and tuple(dev.frames.shape) == (2, 62, 64, 64, 3) and torch.equal(dev.frames, host.frames)


def test_generate_under_the_environment_variable_writes_the_host_routes_files(tmp_path, monkeypatch):
    trees = {d: I.write_raw_tree(tmp_path / d, 2, 5) for d in ('device', 'host')}
    for d, tree in trees.items():
        monkeypatch.setenv(C.DECODE_ENV, d)
        assert gen_chairs.generate(tree, 64, torch.device(DEV), box=I.RAW_BOX) == 10
    for name in I.raw_object_names(2):
        for i in range(5):
            a, b = (open(os.path.join(t, 'rendered_chairs', name, 'renders', '%d.png' % i), 'rb').read() for t in trees.values())
            assert a == b, (name, i)


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('misalign', [0, 1])
def test_neither_entry_writes_outside_its_outputs(monkeypatch, corpus, payload, misalign):
    """Guard bands round out, status, produced and pixels; misalign=1 makes each an offset view one element off its allocation (the
    output slots then start at odd addresses), and the packed input starts at an odd address."""
    allocs = G.guarded_ops(monkeypatch, misalign=misalign)
    small = [(s, p) for _, s, p in corpus if len(p) <= 70000]
    damaged = P.damaged_streams(payload)
    streams = [s for s, _ in small] + [s for s, _ in damaged.values()]
    lengths = [len(p) for _, p in small] + [len(payload)] * len(damaged)
    stride = max(lengths) + 5
    packed, offsets = _pack(streams, lead=3)
    assert packed.data_ptr() % 2 == 1
    out, status, produced = ops.inflate_zlib(packed, offsets, torch.tensor(lengths, dtype=torch.int64, device=DEV), stride)
    assert len(allocs.guards) == 3 and out.data_ptr() % 2 == misalign
    allocs.check()
    for i, (s, p) in enumerate(small):
        assert int(status[i]) == 0 and out[i, :len(p)].cpu().numpy().tobytes() == p
    # bytes of a slot beyond out_len stay untouched (the canary)
    host = out.cpu().numpy()
    for i, n in enumerate(lengths):
        assert (host[i, n:] == G.CANARY).all(), i
    # the filters: slots with a stride, one image failed
    h, w = P.PNG_SIZE
    imgs = np.stack([P.sample_image(h, w, 3, seed=i) for i in range(3)])
    raw = np.full((3, h * (1 + 3 * w) + 7), 0xEE, dtype=np.uint8)
    for i in range(3):
        raw[i, :h * (1 + 3 * w)] = np.frombuffer(P.filter_rows(imgs[i], [(y + i) % 5 for y in range(h)]), dtype=np.uint8)
    raw[1, 0] = 9
    st = torch.zeros(3, dtype=torch.int32, device=DEV)
    pixels = ops.png_unfilter(torch.from_numpy(raw).to(DEV)[:, :], st, h, w, 3)
    assert len(allocs.guards) == 4
    allocs.check()
    assert st.cpu().tolist() == [0, P.BAD_FILTER, 0]
    assert np.array_equal(pixels[0].cpu().numpy(), imgs[0]) and np.array_equal(pixels[2].cpu().numpy(), imgs[2])

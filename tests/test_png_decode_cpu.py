"""PNG decoding on the device, the part that needs no GPU: the two entry points' declarations and argument checks, the chunk parser and
the packer, the rule that selects the decoder, the fall-back of a batch with an interlaced file, the fixtures of tests/png_inputs.py
against `read_png_rgb8` and zlib, and the stream logic of the inflate kernel (csrc/vs_inflate_core.h) compiled for the host and run on
the corpus plus 2 000 seeded mutations."""
import ctypes
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

import host_build
import png_inputs as P
import resample_inputs as I
import resample_ref as R
from spatiotemporal_variable_separation_amd import _lib, ops
from spatiotemporal_variable_separation_amd.data import chairs as C
from spatiotemporal_variable_separation_amd.preprocessing.chairs import gen_chairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('vs_inflate_zlib', 'vs_png_unfilter')


def test_entry_points_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, 'include', 'varsep_hip.h')).read()
    lib = _lib.load_library()
    for name in ENTRIES:
        assert re.search(r'\bint %s\(' % name, header)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert 'vs_png.hip' in _lib.SOURCES
    for i, name in enumerate(('OK', 'HEADER', 'BLOCK_TYPE', 'STORED_LEN', 'LENGTHS', 'SYMBOL', 'DISTANCE', 'INPUT', 'OUT_LONG', 'OUT_SHORT',
                              'ADLER')):
        assert re.search(r'#define VS_INFLATE_%s %d\b' % (name, i), header) and getattr(P, name) == i
    assert re.search(r'#define VS_PNG_BAD_FILTER %d\b' % P.BAD_FILTER, header)
    assert set(ops.INFLATE_STATUS) == set(range(1, 12))


def test_entry_points_refuse_null_pointers_and_non_positive_sizes():
    lib = _lib.load_library()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def inflate(packed=p, nbytes=16, offsets=p, n=1, out_len=p, out=p, stride=8, status=p, produced=p):
        return lib.vs_inflate_zlib(packed, nbytes, offsets, n, out_len, out, stride, status, produced, None)

    def unfilter(raw=p, stride=100, n=1, H=3, W=5, C=3, pixels=p, status=p):
        return lib.vs_png_unfilter(raw, stride, n, H, W, C, pixels, status, None)

    for call, name, bad in (
            (inflate, 'vs_inflate_zlib', [dict(packed=None), dict(offsets=None), dict(out_len=None), dict(out=None), dict(status=None),
                                          dict(produced=None), dict(n=0), dict(n=-3), dict(nbytes=-1), dict(stride=0), dict(n=1 << 31)]),
            (unfilter, 'vs_png_unfilter', [dict(raw=None), dict(pixels=None), dict(status=None), dict(n=0), dict(H=0), dict(W=-1), dict(C=0),
                                           dict(C=5), dict(stride=47), dict(W=70000, stride=1 << 40), dict(n=1 << 31)])):
        for kwargs in bad:
            assert call(**kwargs) == -1, (name, kwargs)
            assert name in lib.vs_last_error().decode(), (name, kwargs)
    unfilter(stride=47)
    assert '47' in lib.vs_last_error().decode() and '16' in lib.vs_last_error().decode()      # 3 rows of 16 bytes need 48


def test_ops_refuse_cpu_tensors_and_wrong_operands():
    with pytest.raises(_lib.VarsepHipError):
        ops.inflate_zlib(torch.zeros(8, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), 4)
    with pytest.raises(_lib.VarsepHipError):
        ops.png_unfilter(torch.zeros((1, 48), dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), 3, 5, 3)


# ---- the chunk parser and the packer -----------------------------------------------------------------------------------------------
def test_chunk_parser_and_packer():
    cases = P.png_cases()
    h, w = P.PNG_SIZE
    blobs = [P.png_bytes(img, **kw) for img, kw in cases.values()]
    names = list(cases)
    width, height, packed, offsets = ops.png_pack(blobs, names)
    assert (width, height) == (w, h) and packed.dtype == np.uint8 and offsets.dtype == np.int64 and offsets.shape == (len(blobs) + 1,)
    assert offsets[0] == 0 and offsets[-1] == packed.size and np.all(np.diff(offsets) > 0)
    assert any(int(o) % 4 for o in offsets)                                # streams start at odd offsets
    for i, (img, kw) in enumerate(cases.values()):
        stream = packed[offsets[i]:offsets[i + 1]].tobytes()
        assert zlib.decompress(stream) == P.filter_rows(img, _ftypes(img, kw))
    # a multi-IDAT file packs to the stream of the single-IDAT one
    img, kw = cases['rle_3idat']
    assert P.png_bytes(img, **kw).count(b'IDAT') == 3
    header, idat = C.png_chunks(P.png_bytes(img, **kw), 'x')
    assert header == (w, h, 8, 2, 0, 0, 0) and len(idat) == 3
    one = ops.png_pack([P.png_bytes(img, **dict(kw, n_idat=1))])[2]
    i = names.index('rle_3idat')
    assert np.array_equal(packed[offsets[i]:offsets[i + 1]], one)
    # damaged files are named
    with pytest.raises(ValueError, match=r'cycle: truncated PNG chunk'):
        ops.png_pack([blobs[0], blobs[names.index('cycle')][:-30]], ['a', 'cycle'])
    with pytest.raises(C.PngNotCovered, match='b: not a PNG'):
        ops.png_pack([blobs[0], b'JFIF' + blobs[1]], ['a', 'b'])
    with pytest.raises(ValueError, match='b: PNG without a header'):
        ops.png_pack([blobs[0], P.MAGIC + P.chunk(b'IEND', b'')], ['a', 'b'])
    other = P.png_bytes(P.sample_image(h, w + 1))
    with pytest.raises(ValueError, match=r'b: a %d x %d image among %d x %d ones' % (w + 1, h, w, h)):
        ops.png_pack([blobs[0], other], ['a', 'b'])
    for kw in (dict(interlace=1), dict(colour=0), dict(depth=16), dict(colour=6)):
        with pytest.raises(C.PngNotCovered, match='b: an 8-bit non-interlaced RGB PNG'):
            ops.png_pack([blobs[0], P.png_from_stream(w, h, zlib.compress(b'x'), **kw)], ['a', 'b'])
    with pytest.raises(ValueError):
        ops.png_pack([])


def _ftypes(img, kw):
    f = kw.get('ftypes')
    h = img.shape[0]
    return [y % 5 for y in range(h)] if f is None else (P.adaptive_ftypes(img) if f == 'adaptive' else [f] * h)


def test_read_png_rgb8_still_reads_and_refuses_as_before(tmp_path):
    for name, (img, kw) in P.png_cases().items():
        path = str(tmp_path / (name + '.png'))
        with open(path, 'wb') as f:
            f.write(P.png_bytes(img, **kw))
        assert np.array_equal(C.read_png_rgb8(path), img), name            # the fixtures are right without the GPU
    assert {t for img, kw in P.png_cases().values() for t in _ftypes(img, kw)} == {0, 1, 2, 3, 4}
    assert len(set(P.adaptive_ftypes(P.png_cases()['adaptive_l9'][0]))) >= 3
    bad = str(tmp_path / 'bad.png')
    for body, match in ((b'nothing', 'not a PNG file'), (P.MAGIC + b'\0\0\0\x09IHDRxx', 'truncated PNG chunk'),
                        (P.MAGIC + P.chunk(b'IEND', b''), 'PNG without a header'),
                        (P.png_from_stream(4, 4, zlib.compress(b'x'), interlace=1), '8-bit non-interlaced RGB PNG is expected'),
                        (P.png_from_stream(4, 4, zlib.compress(b'x')), '1 bytes of image data, 52 expected'),
                        (P.png_from_stream(4, 4, zlib.compress(bytes(52))[:-3]), 'bad.png: Error')):
        with open(bad, 'wb') as f:
            f.write(body)
        with pytest.raises(ValueError, match=match):
            C.read_png_rgb8(bad)


def test_corpus_is_valid_and_damaged_streams_are_refused_by_zlib():
    names = [name for name, _, _ in P.corpus()]
    assert len(set(names)) == len(names) >= 18
    for name, stream, payload in P.corpus():
        assert zlib.decompress(stream) == payload, name
    sizes = {name: len(payload) for name, _, payload in P.corpus()}
    assert sizes['empty'] == 0 and sizes['one_byte'] == 1 and sizes['level0_70000'] == 70000 and sizes['zeros_200k'] == 200000
    payload = P.corpus()[3][2][:5000]
    for name, (stream, status) in P.damaged_streams(payload).items():
        got = P.zlib_accepts(stream)
        if name in ('one_more', 'one_less'):                               # valid streams of the wrong length
            assert got is not None and len(got) == len(payload) + (1 if name == 'one_more' else -1)
        else:
            assert got is None, name
        assert status != P.OK


# ---- the decoder rule --------------------------------------------------------------------------------------------------------------
def test_decoder_rule_keyword_over_environment_over_default(monkeypatch):
    gpu, cpu = torch.device('cuda', 0), torch.device('cpu')
    for pil in (None, object()):
        monkeypatch.setattr(C, '_pil_image', lambda pil=pil: pil)
        monkeypatch.delenv(C.DECODE_ENV, raising=False)
        assert C.chairs_decoder(None, gpu) == ('device' if pil is None else 'host')            # the default: PIL missing and a GPU
        assert C.chairs_decoder(None, cpu) == 'host' and C.chairs_decoder(None, None) == 'host'
        assert C.chairs_decoder(None, 'cuda:1') == ('device' if pil is None else 'host')
        monkeypatch.setenv(C.DECODE_ENV, '')
        assert C.chairs_decoder(None, gpu) == ('device' if pil is None else 'host')            # empty counts as unset
        for env in ('host', 'device'):
            monkeypatch.setenv(C.DECODE_ENV, env)
            assert C.chairs_decoder(None, gpu) == env and C.chairs_decoder(None, cpu) == env    # the environment over the default
            for kw in ('host', 'device'):
                assert C.chairs_decoder(kw, gpu) == kw                                          # the keyword over the environment
        monkeypatch.setenv(C.DECODE_ENV, 'gpu')
        with pytest.raises(ValueError, match=C.DECODE_ENV):
            C.chairs_decoder(None, gpu)
        assert C.chairs_decoder('host', gpu) == 'host'
        with pytest.raises(ValueError, match='decode'):
            C.chairs_decoder('fast', gpu)
    assert C.DECODE_ENV == 'VARSEP_CHAIRS_DECODE'


def test_decode_keyword_reaches_prepare_renders(monkeypatch, tmp_path):
    seen = []
    monkeypatch.setattr(C, 'prepare_renders', lambda paths, box, size, device, image_module=None, timings=None, decode=None:
                        seen.append(decode) or torch.zeros((len(paths), size, size, 3), dtype=torch.uint8))
    monkeypatch.setattr(C, 'require_gpu', lambda what, device, hint='': torch.device('cpu'))
    tree = I.write_raw_tree(tmp_path, 1, 2)
    gen_chairs.generate(tree, 8, 'cpu', box=I.RAW_BOX, decode='device')
    gen_chairs.generate(tree, 8, 'cpu', box=I.RAW_BOX)
    assert seen == ['device', None]
    calls = []
    monkeypatch.setattr(C.Chairs, '__init__', lambda self, *a, **kw: calls.append((self.raw_box, self.raw_decode)))
    C.Chairs.from_raw(True, 'd', 2, device='cuda', decode='device')
    C.Chairs.from_raw(True, 'd', 2, device='cuda')
    assert calls == [(C.RAW_BOX, 'device'), (C.RAW_BOX, None)] and C.Chairs.raw_decode is None


# ---- the device route's host part, with the launches replaced --------------------------------------------------------------------
@pytest.fixture()
def standins(monkeypatch):
    """The launches replaced on CPU tensors: `png_decode_packed` by zlib + the built-in reader's arithmetic, the resize by the
    restatement.  Records which route ran."""
    calls = []

    def decode_packed(packed, offsets, H, W, C=3):
        calls.append('device')
        packed, offsets = packed.numpy(), offsets.numpy()
        out = np.zeros((len(offsets) - 1, H, W, C), dtype=np.uint8)
        status = np.zeros(len(offsets) - 1, dtype=np.int32)
        for i in range(len(offsets) - 1):
            try:
                raw = zlib.decompress(packed[offsets[i]:offsets[i + 1]].tobytes())
            except zlib.error:
                status[i] = P.INPUT
                continue
            out[i] = _unfilter(raw, H, W, C)
        return torch.from_numpy(out), torch.from_numpy(status)

    host = C.decode_renders
    monkeypatch.setattr(ops, 'png_decode_packed', decode_packed)
    monkeypatch.setattr(ops, 'resample_lanczos_u8', lambda x, box, size: R.resample_tensor(x, box, size))
    monkeypatch.setattr(C, 'decode_renders', lambda *a, **kw: calls.append('host') or host(*a, **kw))
    return calls


def _unfilter(raw, H, W, channels):
    """The filtered rows back into pixels, through the built-in file reader."""
    import tempfile
    assert channels == 3
    with tempfile.NamedTemporaryFile(suffix='.png') as f:
        f.write(P.png_from_stream(W, H, zlib.compress(raw)))
        f.flush()
        return C.read_png_rgb8(f.name)


def _paths(tree, n_views, k=0):
    d = os.path.join(tree, 'rendered_chairs', I.raw_object_names(k + 1)[k], 'renders')
    return [os.path.join(d, f) for f in I.raw_file_names(n_views)]


def test_device_route_packs_uploads_and_names_failures(tmp_path, standins):
    tree = I.write_raw_tree(tmp_path, 1, 3)
    paths = _paths(tree, 3)
    timings = {}
    got = C.prepare_renders(paths, I.RAW_BOX, 64, 'cpu', None, None, decode='device')
    assert standins == ['device']
    want = C.prepare_renders(paths, I.RAW_BOX, 64, 'cpu', None, None, decode='host')
    assert standins == ['device', 'host'] and torch.equal(got, want)
    assert np.array_equal(got.numpy(), R.resample(I.raw_views(0, 3), I.RAW_BOX, 64))
    # errors name the file first, as on the host route
    with pytest.raises(ValueError, match=r'image_000\.png: the crop box'):
        C.prepare_renders(paths, (20, 20, 100, 121), 64, 'cpu', decode='device')
    with pytest.raises(ValueError, match='empty'):
        C.prepare_renders(paths, (20, 20, 20, 100), 64, 'cpu', decode='device')
    with pytest.raises(ValueError, match=r'nothing\.png: missing'):
        C.prepare_renders(paths + [os.path.join(tree, 'nothing.png')], I.RAW_BOX, 64, 'cpu', decode='device')
    small = _paths(I.write_raw_tree(tmp_path / 'small', 1, 1, size=90), 1)
    with pytest.raises(ValueError, match=r'small.*image_000\.png: a 90 x 90 image among 120 x 120 ones'):
        C.prepare_renders(paths + small, I.RAW_BOX, 64, 'cpu', decode='device')
    raw = open(paths[1], 'rb').read()
    with open(paths[1], 'wb') as f:                                        # the stream cut short inside a complete IDAT chunk
        header, idat = C.png_chunks(raw, paths[1])
        f.write(P.png_from_stream(header[0], header[1], b''.join(idat)[:-9]))
    with pytest.raises(ValueError, match=r'image_001\.png: compressed data ends early'):
        C.prepare_renders(paths, I.RAW_BOX, 64, 'cpu', decode='device')


def test_a_batch_with_an_interlaced_file_takes_the_host_route(tmp_path, standins, monkeypatch):
    tree = I.write_raw_tree(tmp_path, 1, 3)
    paths = _paths(tree, 3)
    with open(paths[2], 'wb') as f:                                        # a valid kind of PNG that the kernels do not cover
        f.write(P.png_from_stream(I.RAW_SIZE, I.RAW_SIZE, zlib.compress(b'x'), interlace=1))
    host_calls = []
    monkeypatch.setattr(C, 'decode_renders', lambda p, box, image_module=None:
                        host_calls.append(list(p)) or np.zeros((len(p), I.RAW_SIZE, I.RAW_SIZE, 3), dtype=np.uint8))
    out = C.prepare_renders(paths, I.RAW_BOX, 64, 'cpu', decode='device')
    assert host_calls == [paths] and standins == []                        # the WHOLE batch, and nothing was launched for it
    assert tuple(out.shape) == (3, 64, 64, 3)


def test_generate_takes_the_decoder_from_the_environment(tmp_path, standins, monkeypatch):
    monkeypatch.setattr(C, 'require_gpu', lambda what, device, hint='': torch.device('cpu'))
    tree_d, tree_h = I.write_raw_tree(tmp_path / 'd', 2, 3), I.write_raw_tree(tmp_path / 'h', 2, 3)
    monkeypatch.setenv(C.DECODE_ENV, 'device')
    assert gen_chairs.generate(tree_d, 32, 'cpu', box=I.RAW_BOX) == 6
    monkeypatch.setenv(C.DECODE_ENV, 'host')
    assert gen_chairs.generate(tree_h, 32, 'cpu', box=I.RAW_BOX) == 6
    assert standins == ['device', 'host']
    for name in I.raw_object_names(2):
        for i in range(3):
            a, b = (C.read_png_rgb8(os.path.join(t, 'rendered_chairs', name, 'renders', '%d.png' % i)) for t in (tree_d, tree_h))
            assert np.array_equal(a, b)


# ---- the stream logic of the kernel on the host ---------------------------------------------------------------------------------
def _compile_host_check(tmp_path):
    """tests/host/inflate_host_check.cpp.  (exe, sanitized)."""
    return host_build.compile_host_check(tmp_path, 'inflate_host_check')


def test_inflate_core_on_the_host_agrees_with_zlib_on_the_corpus_and_2000_mutations(tmp_path):
    exe, sanitized = _compile_host_check(tmp_path)
    limit = 1 << 20                                                        # the output limit of a stream zlib refuses
    records = [(s, p) for _, s, p in P.corpus()]
    payload = P.corpus()[3][2][:5000]
    records += [(s, P.zlib_accepts(s)) for s, _ in P.damaged_streams(payload).values()]
    mutated = P.mutations(2000)
    assert len(mutated) == 2000
    records += [(s, P.zlib_accepts(s)) for s in mutated]
    n_ok = sum(p is not None for _, p in records)
    assert n_ok >= len(P.corpus()) + 2 and len(records) - n_ok >= 1000      # both verdicts occur in numbers
    corpus = str(tmp_path / 'corpus.bin')
    with open(corpus, 'wb') as f:
        f.write(struct.pack('<q', len(records)))
        for s, p in records:
            f.write(struct.pack('<qqq', len(s), limit if p is None else len(p), int(p is not None)) + s + (p or b''))
    r = subprocess.run([exe, corpus], capture_output=True, text=True, timeout=600)
    print('sanitizers:', sanitized, '|', r.stdout.strip().splitlines()[-1] if r.stdout.strip() else r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().splitlines()[-1] == 'records %d accepted %d refused %d mismatches 0' % (len(records), n_ok, len(records) - n_ok), \
        r.stdout[-3000:]

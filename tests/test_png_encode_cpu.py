"""PNG encoding on the device, the part that needs no GPU: the three entry points' declarations and argument checks, the wrappers'
refusals, the rule that selects the encoder, the unchanged host route of `generate`, and the encoder's logic
(csrc/vs_png_encode_core.h on top of the two DEFLATE cores) compiled for the host and run on the cases of tests/png_encode_inputs.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import png_encode_inputs as E
import png_inputs as P
import resample_inputs as I
from spatiotemporal_variable_separation_amd import _lib, ops
from spatiotemporal_variable_separation_amd.data import chairs as C
from spatiotemporal_variable_separation_amd.preprocessing.chairs import gen_chairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('vs_png_filter', 'vs_deflate_streams', 'vs_png_assemble')


def test_entry_points_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, 'include', 'varsep_hip.h')).read()
    lib = _lib.load_library()
    for name in ENTRIES:
        assert re.search(r'\bint %s\(' % name, header)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert 'vs_png_encode.hip' in _lib.SOURCES
    assert [len(_lib.SIGNATURES[name][1]) for name in ENTRIES] == [9, 12, 14]
    core = os.path.join(ROOT, 'spatiotemporal_variable_separation_amd', 'csrc', 'vs_png_encode_core.h')
    assert os.path.exists(core) and 'vs_png_encode_core.h' in open(os.path.join(os.path.dirname(core), 'vs_png_encode.hip')).read()
    assert ops.PNG_FIXED_BYTES == E.FIXED_BYTES == 57 + 8 and ops.DEFLATE_SLOT_EXTRA == E.SLOT_EXTRA


def test_entry_points_refuse_what_the_header_lists():
    lib = _lib.load_library()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 2)

    def png_filter(pixels=p, n=1, H=3, W=5, C=3, mode=5, raw=p, stride=48):
        return lib.vs_png_filter(pixels, n, H, W, C, mode, raw, stride, None)

    def streams(src=p, n=2, nbytes=100, stride=128, chunk=1024, match=0, slots=p, slot_stride=1034, sizes=p, work=None, work_bytes=0):
        return lib.vs_deflate_streams(src, n, nbytes, stride, chunk, match, slots, slot_stride, sizes, work, work_bytes, None)

    def assemble(raw=p, raw_stride=48, slots=p, slot_stride=1034, sizes=p, n=1, H=3, W=5, C=3, K=1, files=p, file_stride=65 + 48 + 10, file_bytes=p):
        return lib.vs_png_assemble(raw, raw_stride, slots, slot_stride, sizes, n, H, W, C, K, files, file_stride, file_bytes, None)

    group = 4 * 32768
    for call, name, bad in (
            (png_filter, 'vs_png_filter', [dict(pixels=None), dict(raw=None), dict(n=0), dict(n=-2), dict(H=0), dict(W=-1), dict(C=0), dict(C=5),
                                           dict(mode=-1), dict(mode=6), dict(stride=47), dict(W=65536, C=1, stride=1 << 40),
                                           dict(W=16384, C=4, stride=1 << 40), dict(n=1 << 31, H=8, stride=1 << 40), dict(n=1 << 33)]),
            (streams, 'vs_deflate_streams', [dict(src=None), dict(slots=None), dict(sizes=None), dict(n=0), dict(n=-1), dict(nbytes=0), dict(nbytes=-5),
                                             dict(stride=99), dict(chunk=1023), dict(chunk=32769), dict(match=-1), dict(match=2),
                                             dict(slot_stride=1033), dict(n=1 << 31), dict(n=1 << 30, nbytes=2048, stride=2048),
                                             dict(match=1), dict(match=1, work=p, work_bytes=group - 1),
                                             dict(match=1, work=odd, work_bytes=4 * group)]),
            (assemble, 'vs_png_assemble', [dict(raw=None), dict(slots=None), dict(sizes=None), dict(files=None), dict(file_bytes=None), dict(n=0),
                                           dict(H=0), dict(W=0), dict(K=0), dict(K=-1), dict(slot_stride=0), dict(C=0), dict(C=5),
                                           dict(raw_stride=47), dict(file_stride=65 + 48 + 10 - 1), dict(K=2), dict(K=49, file_stride=1 << 20),
                                           dict(H=32768, W=16383, C=4, K=1 << 16, raw_stride=1 << 40, file_stride=1 << 40),
                                           dict(n=1 << 31)])):
        for kwargs in bad:
            assert call(**kwargs) == -1, (name, kwargs)
            assert name in lib.vs_last_error().decode(), (name, kwargs)
    png_filter(stride=47)
    assert '47' in lib.vs_last_error().decode() and '16' in lib.vs_last_error().decode()          # 3 rows of 16 bytes need 48
    assemble(file_stride=122)
    assert '122' in lib.vs_last_error().decode() and '48' in lib.vs_last_error().decode()         # 57 + 8 + 48 + 10 * 1 = 123
    assemble(H=32768, W=16383, C=4, K=1 << 16, raw_stride=1 << 40, file_stride=1 << 40)
    assert '2^31' in lib.vs_last_error().decode()


def test_ops_refuse_cpu_tensors_and_wrong_operands():
    img = torch.zeros((2, 3, 5, 3), dtype=torch.uint8)
    for call in (lambda: ops.png_filter(img), lambda: ops.deflate_streams(torch.zeros((2, 48), dtype=torch.uint8), 48),
                 lambda: ops.png_encode_u8(img),
                 lambda: ops.png_assemble(torch.zeros((2, 48), dtype=torch.uint8), torch.zeros((2, 1040), dtype=torch.uint8),
                                          torch.zeros(2, dtype=torch.int64), 3, 5, 3)):
        with pytest.raises(_lib.VarsepHipError, match='no CPU fallback'):
            call()


def test_ops_refuse_wrong_dtypes_ranks_and_names(monkeypatch):
    monkeypatch.setattr(ops, 'require_cuda', lambda *t: None)              # the operand checks come before any launch
    good = torch.zeros((2, 3, 5, 3), dtype=torch.uint8)
    for bad in (good.float(), good[0], good[:, :, :, :0], torch.zeros((2, 3, 5, 5), dtype=torch.uint8), good[:0]):
        for fn in (ops.png_filter, ops.png_encode_u8):
            with pytest.raises(_lib.VarsepHipError, match='uint8'):
                fn(bad)
    with pytest.raises(_lib.VarsepHipError, match='contiguous'):
        ops.png_filter(good.permute(0, 2, 1, 3))
    for kw in (dict(filter='best'), dict(filter=6), dict(filter=True), dict(match='lz77'), dict(chunk_bytes=1023), dict(chunk_bytes=32769)):
        with pytest.raises(_lib.VarsepHipError, match=list(kw)[0].split('_')[0]):
            ops.png_encode_u8(good, **kw)
    with pytest.raises(_lib.VarsepHipError, match='filter'):
        ops.png_filter(good, 'optimal')
    with pytest.raises(_lib.VarsepHipError, match='out must be'):
        ops.png_filter(good, out=torch.zeros((2, 47), dtype=torch.uint8))
    raw = torch.zeros((2, 48), dtype=torch.uint8)
    for args in ((raw.int(), 48), (raw[0], 48), (raw, 49), (raw, 0), (raw.t(), 2)):
        with pytest.raises(_lib.VarsepHipError, match='deflate_streams'):
            ops.deflate_streams(*args)
    with pytest.raises(_lib.VarsepHipError, match="match='fast'"):
        ops.deflate_streams(raw, 48, match='fast')


# ---- the encoder rule and the host route -----------------------------------------------------------------------------------------
def test_encoder_rule_keyword_over_environment_and_host_by_default(monkeypatch):
    assert C.ENCODE_ENV == 'VARSEP_CHAIRS_ENCODE'
    monkeypatch.delenv(C.ENCODE_ENV, raising=False)
    assert C.chairs_encoder() == 'host' and C.chairs_encoder(None) == 'host'                     # unset: the host, on every machine
    monkeypatch.setenv(C.ENCODE_ENV, '')
    assert C.chairs_encoder() == 'host'                                                          # empty counts as unset
    for env in ('host', 'device'):
        monkeypatch.setenv(C.ENCODE_ENV, env)
        assert C.chairs_encoder() == env
        for kw in ('host', 'device'):
            assert C.chairs_encoder(kw) == kw                                                    # the keyword over the environment
    monkeypatch.setenv(C.ENCODE_ENV, 'gpu')
    with pytest.raises(ValueError, match=r"%s must be 'host' or 'device'" % C.ENCODE_ENV):
        C.chairs_encoder()
    assert C.chairs_encoder('device') == 'device'
    with pytest.raises(ValueError, match=r"encode must be 'host' or 'device'"):
        C.chairs_encoder('fast')


def _standin_resize(monkeypatch):
    monkeypatch.setattr(C, 'require_gpu', lambda what, device, hint='': torch.device('cpu'))
    monkeypatch.setattr(C, 'prepare_renders', lambda paths, box, size, device, image_module=None, timings=None, decode=None:
                        torch.from_numpy(np.stack([P.sample_image(size, size, seed=i) for i in range(len(paths))])))


def test_generate_host_route_writes_what_it_wrote_before(monkeypatch, tmp_path):
    """encode='host' (and no keyword, no variable) is the code of before: the same files byte for byte from PIL's `save` or from
    `write_png_rgb8`, the same timings keys, and no call into the device encoder."""
    _standin_resize(monkeypatch)
    monkeypatch.delenv(C.ENCODE_ENV, raising=False)
    monkeypatch.setattr(ops, 'png_encode_u8', lambda *a, **kw: pytest.fail('the host route must not reach the device encoder'))
    trees = [I.write_raw_tree(tmp_path / tag, 2, 3) for tag in ('plain', 'host', 'want')]
    timings = {}
    assert gen_chairs.generate(trees[0], 16, 'cpu', box=I.RAW_BOX) == 6
    assert gen_chairs.generate(trees[1], 16, 'cpu', box=I.RAW_BOX, encode='host', timings=timings) == 6
    assert set(timings) == {'download', 'write'}                           # (the stand-in of prepare_renders records none of its own)
    image_module = C._pil_image()
    for k, name in enumerate(sorted(I.raw_object_names(2))):         # (a batch lists its objects sorted)
        for i in range(3):
            want = str(tmp_path / 'want.png')
            img = P.sample_image(16, 16, seed=3 * k + i)
            if image_module is not None:
                image_module.fromarray(img).save(want)
            else:
                C.write_png_rgb8(want, img)
            for tree in trees[:2]:
                path = os.path.join(tree, 'rendered_chairs', name, 'renders', '%d.png' % i)
                assert open(path, 'rb').read() == open(want, 'rb').read(), path
                assert np.array_equal(C.read_png_rgb8(path), img)


def test_generate_device_route_downloads_files_and_only_writes(monkeypatch, tmp_path):
    """The device route with the three launches replaced by the host encoder's bytes: `generate` hands the resized batch to
    ops.png_encode_u8, writes files[i, :sizes[i]] and nothing else, and adds timings the 'encode' key."""
    _standin_resize(monkeypatch)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda device=None: None)
    monkeypatch.setattr(gen_chairs, '_save_all', lambda *a: pytest.fail('the device route must not encode on the host'))
    seen = []

    def encode(images, filter='adaptive', match='window', chunk_bytes=None):
        seen.append(tuple(images.shape))
        blobs = [P.png_bytes(img, 'adaptive') for img in images.numpy()]
        files = np.full((len(blobs), max(len(b) for b in blobs) + 9), 0xEE, dtype=np.uint8)
        for i, b in enumerate(blobs):
            files[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        return torch.from_numpy(files), torch.tensor([len(b) for b in blobs], dtype=torch.int64)

    monkeypatch.setattr(ops, 'png_encode_u8', encode)
    tree = I.write_raw_tree(tmp_path / 'device', 2, 3)
    timings = {}
    monkeypatch.setenv(C.ENCODE_ENV, 'device')
    assert gen_chairs.generate(tree, 16, 'cpu', box=I.RAW_BOX, timings=timings) == 6
    assert seen == [(6, 16, 16, 3)] and set(timings) == {'encode', 'download', 'write'}
    for k, name in enumerate(sorted(I.raw_object_names(2))):         # (a batch lists its objects sorted)
        for i in range(3):
            path = os.path.join(tree, 'rendered_chairs', name, 'renders', '%d.png' % i)
            img = P.sample_image(16, 16, seed=3 * k + i)
            assert open(path, 'rb').read() == P.png_bytes(img, 'adaptive') and np.array_equal(C.read_png_rgb8(path), img)
    monkeypatch.setattr(ops, 'png_encode_u8', lambda images, **kw: (torch.zeros((len(images), 80), dtype=torch.uint8),
                                                                    torch.tensor([70, -1, 70, 70, 70, 70])))
    with pytest.raises(RuntimeError, match=r'1\.png: the device encoder left no file'):
        gen_chairs.generate(tree, 16, 'cpu', box=I.RAW_BOX, encode='device')


# ---- the encoder's logic on the host -----------------------------------------------------------------------------------------------
def _host_cases():
    cases = []
    for shape in E.FILTER_SHAPES:
        for mode in range(6):
            cases.append((E.images(3, shape, seed=mode), mode, 1024, ('runs', 'window')[mode % 2]))
    for name, imgs in E.special_images().items():
        cases.append((imgs, E.ADAPTIVE, 1024, 'window'))
    for n, shape, chunk in E.ENCODE_CASES:
        for match in ('runs', 'window'):
            cases.append((E.images(n, shape, seed=n), E.ADAPTIVE, chunk or E.DEFAULT_CHUNK, match))
    return cases


def test_encoder_logic_on_the_host_filters_deflates_and_frames(tmp_path):
    exe, sanitized = E.compile_host_check(tmp_path)
    cases = _host_cases()
    records, stdout = E.run_host_check(exe, cases, tmp_path)
    print('sanitizers:', sanitized, '|', stdout.strip().splitlines()[-1])
    n_images = sum(len(c[0]) for c in cases)
    assert re.fullmatch(r'records %d images %d chunks \d+ refusals %d' % (len(cases), n_images, n_images), stdout.strip().splitlines()[-1]), stdout[-2000:]
    sizes = {}
    for (imgs, mode, chunk, match), (raws, files) in zip(cases, records):
        want = E.filtered(imgs, mode)
        n, h, w, c = imgs.shape
        S, name = h * (1 + w * c), '%s mode %d chunk %d %s' % (imgs.shape, mode, chunk, match)
        for i in range(n):
            assert raws[i] == want[i], (name, i)                           # the rows are the reference's, types included
            E.check_file(files[i], imgs[i], want[i], name)
            assert len(files[i]) <= E.FIXED_BYTES + S + E.SLOT_EXTRA * -(-S // chunk), name
            if c == 3:
                assert np.array_equal(E.read_back(files[i], tmp_path), imgs[i]), name
        sizes[(imgs.shape, mode, chunk, match)] = [len(f) for f in files]
    for (shape, mode, chunk, match), got in sizes.items():                 # per chunk, and so per file, the window parse is never larger
        if match == 'window' and (shape, mode, chunk, 'runs') in sizes:
            assert all(a <= b for a, b in zip(got, sizes[(shape, mode, chunk, 'runs')])), (shape, chunk)
    # the tie rule and the signed reading, stated outright
    special = E.special_images()
    zero_types = [row[0] for row in np.frombuffer(records[len(E.FILTER_SHAPES) * 6 + 1][0][0], dtype=np.uint8).reshape(6, -1)]
    assert zero_types == [0] * 6                                           # all five sums are 0: the lowest type
    assert P.adaptive_ftypes(special['stripes'][1])[0] != 0                # 0x80 / 0x7F: type 0 would cost 127.5 a byte

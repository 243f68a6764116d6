"""Time and size of the device DEFLATE encoder (csrc/vs_deflate.hip) at the reference's size of the Moving-MNIST test set (10 000 stand-in
digits -> 5 000 videos of 100 frames of 64 x 64, as tools/mmnist_testset_bench.py builds them) and on a literal-heavy probe (noisy
gradients): the three launches (vs_deflate_chunks, vs_deflate_pack, vs_crc32) beside a device copy of the same bytes; the compressed size
against host zlib level 6 and level 1 (one stream, one thread: what np.savez_compressed does) and against the same chunks compressed by
zlib on 16 host threads (the fair host baseline); the command line end to end with VARSEP_NPZ_COMPRESS=host and =device, by stage; and
np.load of both files.  Device times are medians over REPS windows of LAUNCHES launches between two events, warm.  Writes the note given
by --out.

    python tools/deflate_bench.py [--out FILE] [--videos N]
"""
import argparse
import os
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import mmnist_testset_inputs as I  # noqa: E402
from spatiotemporal_variable_separation_amd import _lib, ops  # noqa: E402
from spatiotemporal_variable_separation_amd.data.moving_mnist import synthetic_digits  # noqa: E402
from spatiotemporal_variable_separation_amd.preprocessing.mnist import make_test_set  # noqa: E402
from spatiotemporal_variable_separation_amd.utils import npz  # noqa: E402

N_IMAGES, T, F, ND, SPEED, SEED = 10000, 100, 64, 2, 4, 42
REPS, LAUNCHES = 5, 3
THREADS = 16
L = ops.DEFLATE_CHUNK

lines = []


def say(s=''):
    print(s, flush=True)
    lines.append(s)


def windows_ms(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / LAUNCHES)
    return float(np.median(ts)), min(ts), max(ts)


def zlib_one_stream(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    """(bytes, seconds) of one raw stream on one thread, fed 64 MiB at a time."""
    t0 = time.perf_counter()
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    n = 0
    for lo in range(0, data.size, 64 << 20):
        n += len(co.compress(data[lo:lo + (64 << 20)]))
    n += len(co.flush())
    return n, time.perf_counter() - t0


def zlib_chunks_threads(data, level, keep=False):
    """The encoder's own chunks, each compressed on its own and closed with a sync flush, on THREADS threads (zlib releases the interpreter
    lock): (bytes, seconds, pieces or None).  Every thread takes a contiguous range of chunks."""
    n_chunks = -(-data.size // L)
    per = -(-n_chunks // (THREADS * 8))

    def work(first):
        out = []
        for c in range(first, min(first + per, n_chunks)):
            co = zlib.compressobj(level, zlib.DEFLATED, -15)
            out.append(co.compress(data[c * L:(c + 1) * L]) + co.flush(zlib.Z_SYNC_FLUSH))
        return b''.join(out)

    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=THREADS) as ex:
        pieces = list(ex.map(work, range(0, n_chunks, per)))
    return sum(len(p) for p in pieces), time.perf_counter() - t0, pieces if keep else None


def device_table(name, t, host):
    """The launches on the device tensor t (uint8) and the sizes against host zlib on the same bytes (host: the uint8 array)."""
    lib = _lib.load_library()
    n = t.numel()
    stride = (L + ops.DEFLATE_SLOT_EXTRA + 15) // 16 * 16
    n_chunks = -(-n // L)
    slots = torch.empty((n_chunks, stride), dtype=torch.uint8, device=t.device)
    sizes = torch.empty((n_chunks,), dtype=torch.int64, device=t.device)
    copy = torch.empty_like(t)
    pieces = -(-n // ops.CRC_PIECE)
    partial = torch.empty((pieces,), dtype=torch.int32, device=t.device)

    def deflate():
        _lib.check(lib.vs_deflate_chunks(t.data_ptr(), n, L, slots.data_ptr(), stride, sizes.data_ptr(), _lib.stream_ptr()), 'vs_deflate_chunks')

    deflate()
    ends = torch.cumsum(sizes, 0)
    offsets = ends - sizes
    total = int(ends[-1].item())
    packed = torch.empty((total,), dtype=torch.uint8, device=t.device)

    def pack():
        _lib.check(lib.vs_deflate_pack(slots.data_ptr(), stride, sizes.data_ptr(), offsets.data_ptr(), n_chunks, packed.data_ptr(), total,
                                       _lib.stream_ptr()), 'vs_deflate_pack')

    def crc():
        _lib.check(lib.vs_crc32(t.data_ptr(), n, ops.CRC_PIECE, 0, partial.data_ptr(), _lib.stream_ptr()), 'vs_crc32')

    say('## %s: %d bytes (%.3f GB), %d chunks of %d bytes' % (name, n, n / 1e9, n_chunks, L))
    say()
    say('| launch | time per launch, median (min - max) | input bytes per second |')
    say('|---|---|---|')
    for label, fn in (('vs_deflate_chunks (one wave per chunk, one wave per workgroup)', deflate), ('vs_deflate_pack (%d bytes out)' % total, pack),
                      ('vs_crc32 (one wave per %d bytes, four waves per workgroup)' % ops.CRC_PIECE, crc),
                      ('device copy of the input (`copy_`)', lambda: copy.copy_(t))):
        ms = windows_ms(fn)
        say('| %s | %.3f ms (%.3f - %.3f) | %.1f GB/s |' % (label, ms[0], ms[1], ms[2], n / ms[0] / 1e6))
    pack()
    crc()
    torch.cuda.synchronize()
    stream = packed.cpu().numpy().tobytes() + b'\x03\x00'
    got_crc = int(np.bitwise_xor.reduce(partial.cpu().numpy().view(np.uint32))) ^ 0xFFFFFFFF
    t0 = time.perf_counter()
    d = zlib.decompressobj(-15)
    back, crc_back, at = 0, 0, 0
    for lo in range(0, len(stream), 16 << 20):                             # inflate and compare piece by piece
        out = d.decompress(stream[lo:lo + (16 << 20)])
        same = out == host[at:at + len(out)].tobytes()
        back += len(out) if same else 0
        crc_back = zlib.crc32(out, crc_back)
        at += len(out)
    inflate_s = time.perf_counter() - t0
    say()
    say('* zlib inflates the stream to the input (%d of %d bytes equal, end of stream %s) in %.2f s; vs_crc32 gives %08x, zlib.crc32 %08x.'
        % (back, n, d.eof, inflate_s, got_crc, crc_back))
    say()
    say('| encoder | compressed bytes | against level 6, one stream | host time |')
    say('|---|---|---|---|')
    l6, l6_s = zlib_one_stream(host, 6)
    l1, l1_s = zlib_one_stream(host, 1)
    hf, hf_s = zlib_one_stream(host, 6, zlib.Z_HUFFMAN_ONLY)
    c6, c6_s, _ = zlib_chunks_threads(host, 6)
    c1, c1_s, _ = zlib_chunks_threads(host, 1)
    say('| device: runs at distance 1, stored / fixed / dynamic per %d-byte chunk | %d | %.3f | - |' % (L, len(stream), len(stream) / l6))
    say('| zlib level 6, one stream, one thread (what np.savez_compressed does) | %d | 1.000 | %.2f s |' % (l6, l6_s))
    say('| zlib level 1, one stream, one thread | %d | %.3f | %.2f s |' % (l1, l1 / l6, l1_s))
    say('| zlib Z_HUFFMAN_ONLY, one stream, one thread | %d | %.3f | %.2f s |' % (hf, hf / l6, hf_s))
    say('| zlib level 6, the same %d-byte chunks, %d threads | %d | %.3f | %.2f s |' % (L, THREADS, c6, c6 / l6, c6_s))
    say('| zlib level 1, the same %d-byte chunks, %d threads | %d | %.3f | %.2f s |' % (L, THREADS, c1, c1 / l6, c1_s))
    say()
    del slots, packed, copy


def end_to_end(tmp, images, labels, dev, n_videos):
    I.write_t10k(tmp, images, labels)
    path = {k: os.path.join(tmp, k + '.npz') for k in ('host', 'device', 'host16_l6', 'host16_l1')}
    say('## The command line end to end (%d videos x %d frames), by stage, same box, same run' % (n_videos, T))
    say()
    say('| route | read | draws | launch | download | compress + write | total | file |')
    say('|---|---|---|---|---|---|---|---|')
    for order in ('device', 'host', 'device', 'host'):                     # alternating; every run is reported
        st = {}
        t0 = time.perf_counter()
        if order == 'host':
            arrays = make_test_set.generate(tmp, T, SEED, ND, F, SPEED, dev, timings=st)
            down = st['download']
            make_test_set.save_test_set(path['host'], arrays, 'host', timings=st)
        else:
            arrays = make_test_set.generate_device(tmp, T, SEED, ND, F, SPEED, dev, timings=st)
            make_test_set.save_test_set(path['device'], arrays, 'device', timings=st)
            down = 0.0
        total = time.perf_counter() - t0
        say('| VARSEP_NPZ_COMPRESS=%s | %.2f s | %.2f s | %.4f s | %s | %.2f s | **%.2f s** | %.1f MB |'
            % (order, st['read'], st['draw'], st['kernel'], '%.2f s' % down if order == 'host' else '(compressed bytes only, in the next column)',
               st['write'], total, os.path.getsize(path[order]) / 1e6))
        del arrays
    # the fair host baseline as a route: the download, the same chunks on 16 threads, the same container
    for level in (6, 1):
        st = {}
        t0 = time.perf_counter()
        arrays = make_test_set.generate(tmp, T, SEED, ND, F, SPEED, dev, timings=st)
        t1 = time.perf_counter()
        members = []
        for k, v in arrays.items():
            header = npz.npy_header(v.shape, v.dtype)
            data = np.ascontiguousarray(v).reshape(-1).view(np.uint8)
            _, _, pieces = zlib_chunks_threads(data, level, keep=True)
            members.append(npz.Member(k + '.npy', header, pieces, zlib.crc32(data, zlib.crc32(header)), data.size))
        key = 'host16_l%d' % level
        npz.write_npz(path[key], members)
        total = time.perf_counter() - t0
        say('| host, zlib level %d on %d threads over the same chunks (CRC on one thread included) | %.2f s | %.2f s | %.4f s | %.2f s | %.2f s | **%.2f s** | '
            '%.1f MB |' % (level, THREADS, st['read'], st['draw'], st['kernel'], st['download'], time.perf_counter() - t1, total,
                           os.path.getsize(path[key]) / 1e6))
        del arrays, members
    say()
    say('| np.load of every array of the file | seconds | equal to the host route\'s arrays |')
    say('|---|---|---|')
    with np.load(path['host']) as z:
        t0 = time.perf_counter()
        want = {k: z[k] for k in z.files}
        host_s = time.perf_counter() - t0
    say('| VARSEP_NPZ_COMPRESS=host | %.2f s | - |' % host_s)
    for key in ('device', 'host16_l6', 'host16_l1'):
        with np.load(path[key]) as z:
            t0 = time.perf_counter()
            got = {k: z[k] for k in z.files}
            s = time.perf_counter() - t0
        same = list(got) == list(want) and all(got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]) for k in want)
        say('| %s | %.2f s | %s |' % (key, s, same))
        del got
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'deflate_timing.md'))
    ap.add_argument('--videos', type=int, default=N_IMAGES // ND, help='videos of the set (the reference: 5 000)')
    ap.add_argument('--probe-images', type=int, default=256, help='512 x 512 noisy gradients of the literal-heavy probe')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    n_images = args.videos * ND
    images = synthetic_digits(n_images, seed=SEED)
    labels = (np.arange(n_images) % 10).astype(np.uint8)
    say('# The device DEFLATE encoder at the size of the Moving-MNIST test set (one MI355X, `tools/deflate_bench.py`)')
    say()
    say('Device times: median (min - max) per launch over %d windows of %d launches between two events, warm.  Host times: one run each, '
        'wall clock, on the same box in the same run; at most %d host threads.' % (REPS, LAUNCHES, THREADS))
    say()
    with tempfile.TemporaryDirectory() as tmp:
        I.write_t10k(tmp, images, labels)
        arrays = make_test_set.generate_device(tmp, T, SEED, ND, F, SPEED, dev)
        frames = arrays['sequences'].reshape(-1)
        device_table('Moving-MNIST test videos', frames, frames.cpu().numpy())
        del arrays, frames
        torch.cuda.empty_cache()
        y, x = np.mgrid[0:512, 0:512]
        noise = np.random.RandomState(1).randint(-2, 3, size=(args.probe_images, 512, 512))
        probe = np.clip((x + y)[None] // 8 + noise, 0, 255).astype(np.uint8).reshape(-1)
        device_table('Literal-heavy probe (gradient (x + y) // 8 with +-2 noise)', torch.from_numpy(probe).to(dev), probe)
        torch.cuda.empty_cache()
        end_to_end(tmp, images, labels, dev, args.videos)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

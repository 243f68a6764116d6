"""Seeded inputs of the PNG decoding tests (tests/test_png_decode_cpu.py, tests/test_png_decode_gpu.py): PNG files built from an image
with a chosen filter per row (the filtering done in NumPy here), the zlib streams of the inflate corpus, damaged streams, and seeded
mutations.  Nothing here imports the reference or PIL; `zlib` of the standard library is the parity reference.  The raw render trees are
those of tests/resample_inputs.py."""
import struct
import zlib

import numpy as np

SEED = 8950
MAGIC = b'\x89PNG\r\n\x1a\n'

# status codes of include/varsep_hip.h
OK, HEADER, BLOCK_TYPE, STORED_LEN, LENGTHS, SYMBOL, DISTANCE, INPUT, OUT_LONG, OUT_SHORT, ADLER, BAD_FILTER = range(12)


# ---- PNG files -----------------------------------------------------------------------------------------------------------------
def filter_rows(img, ftypes):
    """bytes of H rows of 1 + W * C: row y of uint8 [H, W, C] filtered with type ftypes[y] (0..4; bpp = C, the row above row 0 is zeros)."""
    h, w, c = img.shape
    rows = img.reshape(h, w * c).astype(np.int32)
    prev = np.zeros(w * c, dtype=np.int32)
    zero = np.zeros(c, dtype=np.int32)
    raw = bytearray()
    for y in range(h):
        cur, f = rows[y], int(ftypes[y])
        left = np.concatenate([zero, cur[:-c]])
        upleft = np.concatenate([zero, prev[:-c]])
        if f == 0:
            pred = np.zeros_like(cur)
        elif f == 1:
            pred = left
        elif f == 2:
            pred = prev
        elif f == 3:
            pred = (left + prev) >> 1
        else:
            p = left + prev - upleft
            pa, pb, pc = np.abs(p - left), np.abs(p - prev), np.abs(p - upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, upleft))
        raw.append(f)
        raw += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(raw)


def adaptive_ftypes(img):
    """The filter type per row an adaptive encoder would choose: the one with the least sum of absolute (signed) residuals."""
    h = img.shape[0]
    cand = [np.frombuffer(filter_rows(img, [f] * h), dtype=np.uint8).reshape(h, -1)[:, 1:].astype(np.int8) for f in range(5)]
    cost = np.stack([np.abs(c.astype(np.int32)).sum(axis=1) for c in cand])
    return [int(f) for f in cost.argmin(axis=0)]


def chunk(kind, body):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body) & 0xffffffff)


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    return co.compress(data) + co.flush()


def png_from_stream(w, h, stream, n_idat=1, colour=2, depth=8, interlace=0):
    """A PNG file around an arbitrary zlib stream, cut into n_idat IDAT chunks."""
    cuts = [len(stream) * i // n_idat for i in range(n_idat + 1)]
    idat = b''.join(chunk(b'IDAT', stream[cuts[i]:cuts[i + 1]]) for i in range(n_idat))
    return MAGIC + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, colour, 0, 0, interlace)) + idat + chunk(b'IEND', b'')


def png_bytes(img, ftypes=None, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, n_idat=1):
    """The bytes of an 8-bit RGB non-interlaced PNG of uint8 [H, W, 3]; ftypes: one type for all rows, a list per row, 'adaptive', or None
    for type (row % 5)."""
    h, w, c = img.shape
    assert c == 3 and img.dtype == np.uint8
    if ftypes is None:
        ftypes = [y % 5 for y in range(h)]
    elif ftypes == 'adaptive':
        ftypes = adaptive_ftypes(img)
    elif isinstance(ftypes, int):
        ftypes = [ftypes] * h
    return png_from_stream(w, h, deflate(filter_rows(img, ftypes), level, strategy), n_idat)


def sample_image(h, w, c=3, seed=0):
    """uint8 [h, w, c]: a smooth gradient, a hard-edged block and a noisy band, so that every filter type has rows it wins."""
    rng = np.random.RandomState(SEED + seed + 131 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 3 + yy * 2 + 17 * k) % 256 for k in range(c)], axis=-1).astype(np.uint8)
    img[h // 4:h // 2 + 1, w // 3:2 * w // 3 + 1] = rng.randint(0, 256, size=(c,))
    band = slice(h // 2, h // 2 + max(h // 5, 1))
    img[band] = rng.randint(0, 256, size=img[band].shape)
    return img


# name -> (image, keyword arguments of png_bytes): one common size, so that they also decode as ONE batch
PNG_SIZE = (37, 53)


def png_cases():
    h, w = PNG_SIZE
    cases = {}
    for f in range(5):
        cases['filter%d' % f] = (sample_image(h, w, seed=f), dict(ftypes=f))
    cases['cycle'] = (sample_image(h, w, seed=5), dict(ftypes=None))
    cases['adaptive_l9'] = (sample_image(h, w, seed=6), dict(ftypes='adaptive', level=9))
    cases['stored'] = (sample_image(h, w, seed=7), dict(ftypes=None, level=0))
    cases['fixed'] = (sample_image(h, w, seed=8), dict(ftypes=4, strategy=zlib.Z_FIXED))
    cases['huffman_only'] = (sample_image(h, w, seed=9), dict(ftypes=3, strategy=zlib.Z_HUFFMAN_ONLY))
    cases['rle_3idat'] = (sample_image(h, w, seed=10), dict(ftypes=1, strategy=zlib.Z_RLE, n_idat=3))
    return cases


# ---- the inflate corpus ----------------------------------------------------------------------------------------------------------
def _text_like(n, rng):
    words = [bytes(rng.randint(97, 123, size=rng.randint(2, 9)).astype(np.uint8)) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += words[rng.randint(0, len(words))] + b' '
    return bytes(out[:n])


def _image_like(n, rng):
    x = np.cumsum(rng.randint(-3, 4, size=n)) + 128
    return (x & 255).astype(np.uint8).tobytes()


def corpus():
    """[(name, zlib stream, payload)]: every stream is valid, and `zlib.decompress(stream) == payload`."""
    rng = np.random.RandomState(SEED)
    text, image = _text_like(100000, rng), _image_like(100000, rng)
    out = [('empty', zlib.compress(b'', 6), b''), ('one_byte', zlib.compress(b'\x5a', 6), b'\x5a')]
    stored = rng.randint(0, 256, size=70000).astype(np.uint8).tobytes()
    out.append(('level0_70000', deflate(stored, 0), stored))                       # 65535 + 4465: two stored blocks
    out.append(('fixed', deflate(text[:20000], 6, zlib.Z_FIXED), text[:20000]))
    for level in (1, 6, 9):
        out.append(('text_l%d' % level, deflate(text, level), text))
        out.append(('image_l%d' % level, deflate(image, level), image))
    out.append(('huffman_only', deflate(image[:30000], 6, zlib.Z_HUFFMAN_ONLY), image[:30000]))
    runs = b''.join(bytes([rng.randint(0, 256)]) * int(rng.randint(200, 3000)) for _ in range(40))
    out.append(('rle_runs', deflate(runs, 6, zlib.Z_RLE), runs))                   # distance 1, length 258
    zeros = bytes(200000)
    out.append(('zeros_200k', deflate(zeros, 9), zeros))
    noise = rng.randint(0, 256, size=65536).astype(np.uint8).tobytes()
    out.append(('random_64k', deflate(noise, 6), noise))
    half = rng.randint(0, 256, size=32768).astype(np.uint8).tobytes()
    out.append(('distance_32768', deflate(half + half, 9), half + half))           # the second half: matches from exactly 32768 back
    co = zlib.compressobj(9, zlib.DEFLATED, 15, 9)
    flushed = co.compress(half) + co.flush(zlib.Z_FULL_FLUSH)
    # after a full flush the encoder has forgotten its history, so the far match across the block boundary is written by hand below
    out.append(('full_flush', flushed + co.compress(half[:5000]) + co.flush(), half + half[:5000]))
    out.append(('far_match_across_blocks', far_match_stream(half), half + half[:258]))
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9)
    sync = b''.join(co.compress(text[i:i + 7000]) + co.flush(zlib.Z_SYNC_FLUSH) for i in range(0, 42000, 7000)) + co.flush()
    out.append(('sync_flush', sync, text[:42000]))
    return out


class BitWriter:
    """LSB-first bit packing, as DEFLATE orders bits; Huffman codes go in MSB first (`code`)."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, count):
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, count):
        for i in range(count - 1, -1, -1):
            self.bits((value >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def fixed_literal(self, v):
        if v < 144:
            self.code(0x30 + v, 8)
        else:
            self.code(0x190 + v - 144, 9)

    def fixed_match(self, length_symbol, length_extra, length_extra_bits, dist_symbol, dist_extra, dist_extra_bits):
        if length_symbol < 280:
            self.code(length_symbol - 256, 7)
        else:
            self.code(0xc0 + length_symbol - 280, 8)
        self.bits(length_extra, length_extra_bits)
        self.code(dist_symbol, 5)
        self.bits(dist_extra, dist_extra_bits)


def _zlib_wrap(deflate_bytes, payload):
    return b'\x78\x9c' + deflate_bytes + struct.pack('>I', zlib.adler32(payload) & 0xffffffff)


def _stored_block(w, data, last):
    w.bits(1 if last else 0, 1)
    w.bits(0, 2)
    w.align()
    w.out += struct.pack('<HH', len(data), len(data) ^ 0xffff) + data


def far_match_stream(half):
    """32768 bytes in one stored block, then a FIXED block whose only symbol is a match of length 258 at distance 32768: the copy crosses the
    block boundary and reaches the very first byte of the output."""
    assert len(half) == 32768
    w = BitWriter()
    _stored_block(w, half, False)
    w.bits(1, 1)
    w.bits(1, 2)
    w.fixed_match(285, 0, 0, 29, 32768 - 24577, 13)
    w.code(0, 7)                                          # end of block
    w.align()
    return _zlib_wrap(bytes(w.out), half + half[:258])


def damaged_streams(payload):
    """{name: (zlib stream, status the decoder must give)} for `payload` (its length is the out_len): each stream is one zlib refuses."""
    good = deflate(payload, 6)
    out = {'truncated': (good[:len(good) // 2], INPUT)}
    w = BitWriter()
    _stored_block(w, payload, True)
    stored = bytearray(_zlib_wrap(bytes(w.out), payload))
    stored[2 + 5 + len(payload) // 2] ^= 0x40             # a byte inside the stored block
    out['adler'] = (bytes(stored), ADLER)
    w = BitWriter()
    w.bits(1, 1)
    w.bits(3, 2)
    w.align()
    out['block_type_3'] = (_zlib_wrap(bytes(w.out), b''), BLOCK_TYPE)
    w = BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    for v in payload[:3]:
        w.fixed_literal(v)
    w.fixed_match(257, 0, 0, 4, 0, 1)                     # length 3 at distance 5 after 3 bytes
    w.code(0, 7)
    w.align()
    out['distance'] = (_zlib_wrap(bytes(w.out), payload), DISTANCE)
    out['fdict'] = (b'\x78\xbb' + good[2:], HEADER)       # FDICT set, check bits right: 0x78bb % 31 == 0
    out['one_more'] = (deflate(payload + b'\x00', 6), OUT_LONG)
    out['one_less'] = (deflate(payload[:-1], 6), OUT_SHORT)
    return out


def zlib_accepts(stream):
    try:
        return zlib.decompress(stream)
    except zlib.error:
        return None


def mutations(count, seed=SEED):
    """`count` seeded mutations of the corpus' smaller streams: a byte flip, a truncation or a splice of two streams."""
    rng = np.random.RandomState(seed)
    base = [s for _, s, p in corpus() if len(s) <= 40000]
    out = []
    for i in range(count):
        s = bytearray(base[rng.randint(0, len(base))])
        kind = i % 3
        if kind == 0 and len(s):
            for _ in range(rng.randint(1, 4)):
                s[rng.randint(0, len(s))] ^= 1 << rng.randint(0, 8)
        elif kind == 1:
            s = s[:rng.randint(0, len(s) + 1)]
        else:
            o = base[rng.randint(0, len(base))]
            s = s[:rng.randint(0, len(s) + 1)] + o[rng.randint(0, len(o) + 1):]
        out.append(bytes(s))
    return out

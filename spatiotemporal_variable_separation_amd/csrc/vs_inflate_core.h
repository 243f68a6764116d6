// vs_inflate_core.h -- the stream logic of vs_inflate_zlib (csrc/vs_png.hip) as plain __host__ __device__ functions: the bit reader, the
// RFC 1950 framing, the three block types of RFC 1951, the construction and validation of the code tables and the decoding of symbols.
// What it does NOT contain is where the bytes go: every byte produced is handed to a SINK (literal, copy from `dist` back, run of stored
// bytes from the input, Adler-32 of everything at the end), which is the kernel's LDS window with its cooperative copy on the device and
// a plain buffer in the host check (tests/host/inflate_host_check.cpp).  The header compiles with a host compiler alone, so the logic
// is exercised on the CPU, under sanitizers, on valid and on damaged streams before it runs on a GPU.
//
// Execution model on the device: ONE WAVE PER STREAM, and every lane runs this code with the same values (same input bytes, same tables),
// so control flow is wave-uniform.  `lane` / `nlanes` only (a) restrict the stores into the shared tables to lane 0 and (b) stripe the fill
// of the first-level lookup tables over the lanes; the host passes lane 0 of 1.  VSI_SYNC() separates a phase that writes the tables from
// one that reads them (a workgroup barrier on the device, nothing on the host).
//
// Termination and bounds, on ANY input:
//   * bits are only ever taken through vsi_take / vsi_drop, which fail with VS_INFLATE_INPUT when the stream has fewer left; the reader
//     never touches a byte outside [in, in + n);
//   * the symbol loop of a block consumes at least one bit per turn or stops with a status; the code-length loop advances its index by at
//     least one per turn up to hlit + hdist <= 316; every other loop has a constant trip count;
//   * a set of code lengths is checked for over-subscription BEFORE a table is built from it, and an incomplete set is accepted only in
//     the form zlib accepts (a single code of one bit); the canonical walk then cannot index past the symbols that exist;
//   * a symbol indexes the base / extra tables only after its range check (length symbols 257..285, distance symbols 0..29);
//   * the sink is called only with pos + len <= out_len and dist <= pos: nothing is written outside the slot, nothing read before it.
// What is accepted and what is refused follows zlib's inflate (the parity reference): trailing bytes after the Adler-32 are ignored,
// more than 286 literal/length or 30 distance codes are refused, a literal/length set without the end-of-block code is refused.
#pragma once
#include <stdint.h>

#include "../../include/varsep_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VSI_HD __host__ __device__ inline
#else
#define VSI_HD inline
#endif
#ifndef VSI_SYNC
#define VSI_SYNC() ((void)0)
#endif

#define VSI_FAST_BITS 9
#define VSI_FAST_SIZE (1 << VSI_FAST_BITS)
#define VSI_MAX_BITS 15
#define VSI_MAX_LIT 288
#define VSI_MAX_LENS 320             /* 286 + 30 of a dynamic header, 288 + 32 of the fixed code */

// One canonical Huffman code: count[l] codes of l bits, their symbols in canonical order, and the first-level lookup
// fast[next VSI_FAST_BITS bits, LSB first] = (symbol << 4) | length for codes of at most VSI_FAST_BITS bits, 0 for longer (or unused) ones.
struct VsiHuff {
    uint16_t count[VSI_MAX_BITS + 1];
    uint16_t symbol[VSI_MAX_LIT];
    uint16_t fast[VSI_FAST_SIZE];
};

struct VsiTables {
    VsiHuff lit, dist;
    uint8_t lens[VSI_MAX_LENS];
};

struct VsiBits {
    const uint8_t* in;
    int64_t n, pos;                    // bytes of the stream, next byte to load
    uint64_t buf;                      // bits not yet consumed, LSB first
    int cnt;                           // how many of them are real (the rest are zeros)
    int err;
};

VSI_HD void vsi_refill(VsiBits& b) {
    if (b.cnt > 32) return;
    if (b.pos + 4 <= b.n) {            // four independent loads in flight, one wait
        const uint8_t* p = b.in + b.pos;
        const uint32_t w = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        b.buf |= (uint64_t)w << b.cnt;
        b.cnt += 32;
        b.pos += 4;
        return;
    }
    while (b.cnt <= 56 && b.pos < b.n) {   // the last three bytes of the stream
        b.buf |= (uint64_t)b.in[b.pos++] << b.cnt;
        b.cnt += 8;
    }
}

// consumes k <= 32 bits that vsi_refill made available; fails (and consumes nothing) when the stream has fewer
VSI_HD void vsi_drop(VsiBits& b, int k) {
    if (k > b.cnt) {
        b.err = VS_INFLATE_INPUT;
        return;
    }
    b.buf >>= k;
    b.cnt -= k;
}

VSI_HD uint32_t vsi_take(VsiBits& b, int k) {   // k in 0..16
    vsi_refill(b);
    const uint32_t v = (uint32_t)b.buf & ((1u << k) - 1u);
    vsi_drop(b, k);
    return v;
}

// The canonical walk over at most max_len bits of `bits` (LSB first): the symbol and its length, or -1 when the bits are no code of h.
VSI_HD int vsi_walk(const VsiHuff* h, uint32_t bits, int max_len, int* len_out) {
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= max_len; ++len) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int cnt = h->count[len];
        if (code - cnt < first) {      // index + (code - first) < index + cnt <= number of symbols: inside symbol[]
            *len_out = len;
            return h->symbol[index + (code - first)];
        }
        index += cnt;
        first += cnt;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

// One symbol of code h from the next bits: the first-level table, then the canonical walk for what it does not hold.
// -1 with b.err set: the stream ended inside the code (VS_INFLATE_INPUT) or the bits are no code of h (VS_INFLATE_SYMBOL).
VSI_HD int vsi_decode(VsiBits& b, const VsiHuff* h) {
    vsi_refill(b);
    const uint32_t bits = (uint32_t)b.buf;
    const uint32_t e = h->fast[bits & (VSI_FAST_SIZE - 1)];
    if (e) {
        vsi_drop(b, (int)(e & 15u));
        return b.err ? -1 : (int)(e >> 4);
    }
    int len = 0;
    const int sym = vsi_walk(h, bits, VSI_MAX_BITS, &len);
    if (sym < 0) {
        b.err = b.cnt < VSI_MAX_BITS ? VS_INFLATE_INPUT : VS_INFLATE_SYMBOL;
        return -1;
    }
    vsi_drop(b, len);
    return b.err ? -1 : sym;
}

// Sixteen 10-bit counters (values <= 288) in three words, six to a word: what a private array indexed at run time would keep in
// scratch memory stays in registers.
struct VsiCounters {
    uint64_t w0, w1, w2;
};
VSI_HD int vsi_counter_get(const VsiCounters& c, int i) {                 // i in 0..15
    const uint64_t w = i < 6 ? c.w0 : (i < 12 ? c.w1 : c.w2);
    return (int)((w >> (10 * (i % 6))) & 1023u);
}
VSI_HD void vsi_counter_add(VsiCounters& c, int i, int v) {               // the sum stays below 1024
    const uint64_t inc = (uint64_t)v << (10 * (i % 6));
    c.w0 += i < 6 ? inc : 0;
    c.w1 += (i >= 6 && i < 12) ? inc : 0;
    c.w2 += i >= 12 ? inc : 0;
}

// Builds code h from lens[0 .. n), n <= VSI_MAX_LIT, every length <= 15.  0, or VS_INFLATE_LENGTHS for an over-subscribed set or an
// incomplete one; with allow_single, zlib's exception is made: a set whose codes all have one bit (a single code) may be incomplete, and
// a set without any code is built (every decode of it then fails).  The return value is uniform; lane 0 stores count[] and symbol[], the
// fill of the first-level table is striped over the lanes.
VSI_HD int vsi_build(VsiHuff* h, const uint8_t* lens, int n, bool allow_single, int lane, int nlanes) {
    VSI_SYNC();                        // lens[] is complete, and nobody still decodes with the previous contents of h
    VsiCounters count = {0, 0, 0};
    for (int s = 0; s < n; ++s) vsi_counter_add(count, lens[s] & 15, 1);
    int left = 1, maxlen = 0;
    bool over = false;
    VsiCounters offs = {0, 0, 0};
    int sum = 0;
    for (int len = 1; len <= VSI_MAX_BITS; ++len) {
        const int c = vsi_counter_get(count, len);
        if (lane == 0) h->count[len] = (uint16_t)c;
        if (c) maxlen = len;
        vsi_counter_add(offs, len, sum);                                   // where the symbols of this length start
        sum += c;
        left <<= 1;
        left -= c;
        if (left < 0) {                // over-subscribed (left is reset: the shifts stay defined)
            over = true;
            left = 0;
        }
    }
    if (over) return VS_INFLATE_LENGTHS;
    if (left > 0 && !(allow_single && maxlen <= 1)) return VS_INFLATE_LENGTHS;   // incomplete
    if (lane == 0) h->count[0] = 0;
    for (int s = 0; s < n; ++s) {
        const int l = lens[s] & 15;
        if (l) {
            const int at = vsi_counter_get(offs, l);                       // < sum of the counts <= n <= VSI_MAX_LIT
            if (lane == 0) h->symbol[at] = (uint16_t)s;
            vsi_counter_add(offs, l, 1);
        }
    }
    VSI_SYNC();
    for (int i = lane; i < VSI_FAST_SIZE; i += nlanes) {
        int len = 0;
        const int sym = vsi_walk(h, (uint32_t)i, VSI_FAST_BITS, &len);
        h->fast[i] = sym >= 0 ? (uint16_t)((sym << 4) | len) : (uint16_t)0;
    }
    VSI_SYNC();
    return 0;
}

VSI_HD int vsi_length_base(int i) {      // i = symbol - 257 in 0..28
    const uint16_t base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    return base[i];
}
VSI_HD int vsi_length_extra(int i) { return i < 8 || i == 28 ? 0 : (i - 4) >> 2; }
VSI_HD int vsi_dist_extra(int i) { return i < 4 ? 0 : (i - 2) >> 1; }       // i in 0..29
VSI_HD int vsi_dist_base(int i) {
    if (i < 4) return i + 1;
    const int e = (i - 2) >> 1;
    return 1 + ((2 + (i & 1)) << e);
}

// The code lengths of a dynamic header (RFC 1951 3.2.7) into t->lens and the two tables from them.
VSI_HD int vsi_dynamic_header(VsiBits& b, VsiTables* t, int lane, int nlanes) {
    const int hlit = (int)vsi_take(b, 5) + 257, hdist = (int)vsi_take(b, 5) + 1, hclen = (int)vsi_take(b, 4) + 4;
    if (b.err) return b.err;
    if (hlit > 286 || hdist > 30) return VS_INFLATE_LENGTHS;
    VSI_SYNC();                        // nobody still reads lens[] of the previous block
    for (int i = 0; i < 19; ++i) {     // the code-length code, in the order of the RFC
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        const uint32_t v = i < hclen ? vsi_take(b, 3) : 0u;
        if (lane == 0) t->lens[order[i]] = (uint8_t)v;
    }
    if (b.err) return b.err;
    int st = vsi_build(&t->lit, t->lens, 19, false, lane, nlanes);      // (the literal table's storage serves the code-length code)
    if (st) return st;
    int idx = 0, prev = 0, eob_len = 0;
    const int total = hlit + hdist;
    while (idx < total) {              // idx advances by at least 1 per turn
        const int sym = vsi_decode(b, &t->lit);
        if (sym < 0) return b.err == VS_INFLATE_SYMBOL ? VS_INFLATE_LENGTHS : b.err;
        int rep = 1, val = sym;
        if (sym == 16) {
            if (idx == 0) return VS_INFLATE_LENGTHS;                        // nothing to repeat
            val = prev;
            rep = 3 + (int)vsi_take(b, 2);
        } else if (sym == 17) {
            val = 0;
            rep = 3 + (int)vsi_take(b, 3);
        } else if (sym == 18) {
            val = 0;
            rep = 11 + (int)vsi_take(b, 7);
        }
        if (b.err) return b.err;
        if (idx + rep > total) return VS_INFLATE_LENGTHS;
        if (idx <= 256 && 256 < idx + rep) eob_len = val;
        if (lane == 0)
            for (int r = 0; r < rep; ++r) t->lens[idx + r] = (uint8_t)val; // idx + r < total <= 316
        idx += rep;
        prev = val;
    }
    if (eob_len == 0) return VS_INFLATE_LENGTHS;                            // no end-of-block code
    st = vsi_build(&t->lit, t->lens, hlit, true, lane, nlanes);
    if (st) return st;
    return vsi_build(&t->dist, t->lens + hlit, hdist, true, lane, nlanes);
}

VSI_HD int vsi_fixed_tables(VsiTables* t, int lane, int nlanes) {
    VSI_SYNC();
    for (int s = lane; s < 320; s += nlanes) t->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
    int st = vsi_build(&t->lit, t->lens, 288, true, lane, nlanes);
    if (st) return st;
    return vsi_build(&t->dist, t->lens + 288, 32, true, lane, nlanes);  // 30 and 31 are coded but never valid
}

// One zlib stream.  Sink: void lit(uint8_t), void copy(int dist, int len), void stored(const uint8_t* src, int len), uint32_t adler();
// the sink appends at its own position, which is `*produced` here.  Returns the status; *produced = bytes handed to the sink.
template <class Sink>
VSI_HD int vsi_inflate_zlib(const uint8_t* in, int64_t n, int64_t out_len, VsiTables* t, Sink& sink, int64_t* produced, int lane, int nlanes) {
    VsiBits b;
    b.in = in; b.n = n; b.pos = 0; b.buf = 0; b.cnt = 0; b.err = 0;
    int64_t pos = 0;
    *produced = 0;
    if (n < 2) return VS_INFLATE_INPUT;
    const uint32_t cmf = vsi_take(b, 8), flg = vsi_take(b, 8);
    if (b.err) return b.err;
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u)) return VS_INFLATE_HEADER;
    int status = 0;
    bool last = false;
    while (!last && !status) {         // every turn consumes the three header bits or stops
        last = vsi_take(b, 1) != 0;
        const uint32_t type = vsi_take(b, 2);
        if (b.err) { status = b.err; break; }
        if (type == 3) { status = VS_INFLATE_BLOCK_TYPE; break; }
        if (type == 0) {
            vsi_drop(b, b.cnt & 7);                                         // to the byte boundary
            const uint32_t len = vsi_take(b, 16), nlen = vsi_take(b, 16);
            if (b.err) { status = b.err; break; }
            if ((len ^ 0xffffu) != nlen) { status = VS_INFLATE_STORED_LEN; break; }
            b.pos -= b.cnt >> 3;                                            // whole bytes the reader holds go back to the stream
            b.buf = 0;
            b.cnt = 0;
            if (b.pos + (int64_t)len > n) { status = VS_INFLATE_INPUT; break; }
            if (pos + (int64_t)len > out_len) { status = VS_INFLATE_OUT_LONG; break; }
            if (len) sink.stored(in + b.pos, (int)len);
            b.pos += len;
            pos += len;
            continue;
        }
        status = type == 1 ? vsi_fixed_tables(t, lane, nlanes) : vsi_dynamic_header(b, t, lane, nlanes);
        while (!status) {              // every turn consumes at least one bit or sets the status
            const int sym = vsi_decode(b, &t->lit);
            if (sym < 0) { status = b.err; break; }
            if (sym < 256) {
                if (pos >= out_len) { status = VS_INFLATE_OUT_LONG; break; }
                sink.lit((uint8_t)sym);
                ++pos;
                continue;
            }
            if (sym == 256) break;
            if (sym > 285) { status = VS_INFLATE_SYMBOL; break; }
            const int li = sym - 257;
            const int len = vsi_length_base(li) + (int)vsi_take(b, vsi_length_extra(li));
            const int ds = vsi_decode(b, &t->dist);
            if (ds < 0) { status = b.err; break; }
            if (ds > 29) { status = VS_INFLATE_SYMBOL; break; }
            const int de = vsi_dist_extra(ds);
            int dist = vsi_dist_base(ds);
            if (de > 8) {                                                   // up to 13 extra bits: two takes keep every take <= 16 of >= 25 buffered
                dist += (int)vsi_take(b, 8);
                dist += (int)vsi_take(b, de - 8) << 8;
            } else {
                dist += (int)vsi_take(b, de);
            }
            if (b.err) { status = b.err; break; }
            if ((int64_t)dist > pos) { status = VS_INFLATE_DISTANCE; break; }
            if (pos + len > out_len) { status = VS_INFLATE_OUT_LONG; break; }
            sink.copy(dist, len);
            pos += len;
        }
    }
    *produced = pos;
    if (status) return status;
    vsi_drop(b, b.cnt & 7);
    uint32_t want = 0;
    for (int i = 0; i < 4; ++i) want = (want << 8) | vsi_take(b, 8);
    if (b.err) return b.err;
    if (want != sink.adler()) return VS_INFLATE_ADLER;
    if (pos < out_len) return VS_INFLATE_OUT_SHORT;
    return VS_INFLATE_OK;
}

// vs_inflate_blocks_core.h -- the logic of csrc/vs_inflate_blocks.hip as plain __host__ __device__ functions on top of csrc/vs_inflate_core.h
// (bit reader, table builder, header parser) and csrc/vs_inflate_chunks_core.h (cells and marks): the parallel decode of a raw RFC 1951 stream
// that is NOT cut at sync markers -- what zlib and therefore np.savez_compressed write.  Every BLOCK of such a stream is a legal place to
// start a decoder; where the blocks start is not stored, it is found.  The header compiles with a host compiler alone
// (tests/host/inflate_blocks_host_check.cpp runs all of it under sanitizers, on valid, on speculative and on damaged input).
//
// 1. THE FINDER (vsb_block_start).  A bit position is a CANDIDATE when a dynamic-Huffman block header that zlib could have written reads
//    from it: BFINAL = 0, BTYPE = 2, HLIT <= 29 and HDIST <= 29; the code-length code is complete (Kraft sum exactly 1); the run-length
//    coded lengths fill HLIT + HDIST entries exactly and repeat code 16 is never first; there is an end-of-block code; the literal/length
//    code is complete; the distance code is complete, or has no code, or one code of one bit (the exception zlib's inflate makes).
//    vsb_quick is the cheap necessary condition (the first 17 bits and the Kraft sum of the code-length code, from 81 bits of the stream)
//    that removes all but about one position in 500 before the full validation.  Nothing is stored per position: the code-length code
//    lives in two packed words, the two sets of lengths only as their counts per length (VsiCounters).  Bit 0 is a candidate always.
//    A false candidate costs a decode that is thrown away and nothing else: see 3.
//    THE STORED FINDER (vsb_stored_boundary, vsb_stored_start; opt-in) adds the positions from which a non-final STORED block header reads:
//    BFINAL = 0, BTYPE = 00 and zero padding up to a byte boundary where LEN and NLEN = ~LEN stand and LEN + 1 more bytes follow.  A
//    boundary gives up to eight adjacent candidates (the padding cannot be told from the header bits); all but one are false, see 3.
//
// 2. A SPAN (vsb_inflate_span) is what one wave decodes: blocks (stored, fixed, dynamic) from a bit offset until
//      * PROBE (cand != null): a block ends at a bit position that is in the sorted candidate list (binary search), or a final block ends;
//        the window before the span is unknown, so a match that reaches before the span's first byte is no error: the byte is EXTERNAL and
//        its cell records VSC_EXT | o, its source being the byte o + 1 before the span's first output byte (csrc/vs_inflate_chunks_core.h).
//        The output is not capped: the sink (VsbRing) is a ring of VSB_WINDOW cells, which is all that a later span can refer to, and the
//        counts of external bytes and their largest reach are kept while decoding, not by a scan at the end;
//      * DECODE (cand == null): a block ends at or after stop_bit, or a final block ends; the `hist` bytes before the span are known (the
//        sink holds them), a distance beyond pos + hist is VS_INFLATE_DISTANCE, more than max_out bytes are VS_INFLATE_OUT_LONG.
//    `end` is the bit position behind the last block consumed (behind the end-of-block code or the last stored byte; not rounded up).
//
// 3. THE CHAIN is walked by the caller from candidate 0: a span's successor is the candidate at its end.  A block end that is a candidate
//    is a true block start by construction (the chain began at bit 0), so false candidates are decoded and ignored and never alter bytes.
//
// 4. WINDOWS (vsb_window_byte).  In chain order, the tail cells of span k and the window before it give the window before span k + 1: a value
//    stays, a mark o reads byte VSB_WINDOW - 1 - o of the previous window, a span shorter than the window keeps the rest of the previous
//    window in front of its own bytes.  Row j of a window is the byte VSB_WINDOW - j before the span's first output byte.
//
// Execution model as in vs_inflate_core.h: one wave per span, every lane runs this code with the same values; `lane` / `nlanes` stripe the
// copies.  VSC_FENCE() orders a phase that writes cells before one that reads them.  vsb_block_start is the exception: ONE LANE PER BIT
// POSITION, every lane with its own reader and nothing shared.
//
// Termination and bounds, on ANY input (false candidates feed garbage on purpose) -- the rules of vs_inflate_chunks_core.h:
//   * the bit reader is vs_inflate_core.h's over [comp, comp + limit), limit = min(comp_bytes, start byte + VSB_MAX_IN): nothing outside the
//     stream is read, and a span reads at most VSB_MAX_IN bytes however the bits go; a span that wants more ends with VS_INFLATE_CAP;
//   * the block loop consumes the three header bits per turn or stops, the symbol loop one bit per turn or stops, the code-length loops
//     advance their index by at least one per turn up to 316; tables are validated before they are built, symbols are range-checked before
//     they index a table; the finder's canonical walk indexes its 19 packed symbols at index + (code - first) < number of codes <= 19;
//   * a ring cell is written at (pos + i) & (VSB_WINDOW - 1) only, a copy reads cell s & (VSB_WINDOW - 1) only for 0 <= s < pos with
//     pos - s <= 32768 (a distance is at most 32768: distance symbols above 29 are refused), and forms VSC_EXT | (-s - 1) <= 32767 for s < 0;
//   * the decode sink is called only with pos + len <= max_out and dist <= pos + hist.
#pragma once
#include "vs_inflate_chunks_core.h"

#ifndef VSB_WAVE_SUM64
#define VSB_WAVE_SUM64(v) (v)
#endif

#define VSB_WINDOW VS_INFLATE_WINDOW_BYTES          /* cells of the probe's ring, bytes of a window */
#define VSB_MASK (VSB_WINDOW - 1)
#define VSB_MAX_IN VS_INFLATE_BLOCKS_MAX_IN         /* bytes of input a span may read */
#define VSB_QUICK_BITS 81                           /* bits of the stream vsb_quick looks at (17 + 3 * 19, and up to 7 of the shift) */

// ---- 1. the finder -------------------------------------------------------------------------------------------------------------------
// The cheap necessary condition.  w: the 64 bits of the stream from the position (LSB first), hi: the 32 bits behind them; zeros beyond the end.
VSI_HD bool vsb_quick(uint64_t w, uint32_t hi) {
    if ((w & 7u) != 4u) return false;                                       // BFINAL = 0, BTYPE = 2
    if (((w >> 3) & 31u) > 29u || ((w >> 8) & 31u) > 29u) return false;
    const int hclen = (int)((w >> 13) & 15u) + 4;
    const uint64_t cl = (w >> 17) | ((uint64_t)hi << 47);                   // 3 bits per code-length code length, 57 at most
    int kraft = 0;
    for (int i = 0; i < 19; ++i) {
        const int l = i < hclen ? (int)((cl >> (3 * i)) & 7u) : 0;
        kraft += l ? 128 >> l : 0;
    }
    return kraft == 128;
}

// 64 bits of comp[0 .. n) from bit position `bit` >= 0 and the 32 behind them, zeros beyond the end (the one-position form of what the scan
// kernel does with a thread's own bytes).
VSI_HD void vsb_peek(const uint8_t* comp, int64_t n, int64_t bit, uint64_t* w, uint32_t* hi) {
    const int64_t p = bit >> 3;
    const int s = (int)(bit & 7);
    uint64_t a = 0, c = 0;
    for (int k = 0; k < 8; ++k) {
        if (p + k < n) a |= (uint64_t)comp[p + k] << (8 * k);
        if (p + 8 + k < n && k < 5) c |= (uint64_t)comp[p + 8 + k] << (8 * k);
    }
    *w = s ? (a >> s) | (c << (64 - s)) : a;
    *hi = (uint32_t)(c >> s);
}

VSI_HD int vsb_sym5(uint64_t s0, uint64_t s1, int i) {                      // the i-th of 19 packed 5-bit symbols, i in 0..18
    return (int)(((i < 12 ? s0 >> (5 * i) : s1 >> (5 * (i - 12)))) & 31u);
}

// The full rule: whether a block header as described at the head of this file reads from bit position `bit` of comp[0 .. n).
VSI_HD bool vsb_block_start(const uint8_t* comp, int64_t n, int64_t bit) {
    if (bit < 0 || (bit >> 3) >= n) return false;
    VsiBits b;
    b.in = comp; b.n = n; b.pos = bit >> 3; b.buf = 0; b.cnt = 0; b.err = 0;
    vsi_take(b, (int)(bit & 7));
    if (vsi_take(b, 3) != 4u) return false;
    const int hlit = (int)vsi_take(b, 5) + 257, hdist = (int)vsi_take(b, 5) + 1, hclen = (int)vsi_take(b, 4) + 4;
    if (b.err || hlit > 286 || hdist > 30) return false;
    uint64_t cl = 0, cnt = 0;              // cl: 3 bits per symbol of the code-length code, its length; cnt: 5 bits per length, how many have it
    int kraft = 0;
    for (int i = 0; i < 19; ++i) {
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        const uint32_t v = i < hclen ? vsi_take(b, 3) : 0u;
        cl |= (uint64_t)v << (3 * order[i]);
        if (v) {
            cnt += (uint64_t)1 << (5 * v);
            kraft += 128 >> v;
        }
    }
    if (b.err || kraft != 128) return false;
    uint64_t s0 = 0, s1 = 0;               // the symbols in canonical order, 5 bits each
    int k = 0;
    for (int l = 1; l <= 7; ++l)
        for (int s = 0; s < 19; ++s)
            if ((int)((cl >> (3 * s)) & 7u) == l) {
                if (k < 12) s0 |= (uint64_t)s << (5 * k); else s1 |= (uint64_t)s << (5 * (k - 12));
                ++k;
            }
    VsiCounters lc = {0, 0, 0}, dc = {0, 0, 0};                             // codes per length of the two sets
    int idx = 0, prev = 0, eob_len = 0;
    const int total = hlit + hdist;
    while (idx < total) {                  // idx advances by at least 1 per turn
        vsi_refill(b);
        uint32_t bits = (uint32_t)b.buf;
        int code = 0, first = 0, index = 0, sym = -1, len = 1;
        for (; len <= 7; ++len) {
            code |= (int)(bits & 1u);
            bits >>= 1;
            const int c = (int)((cnt >> (5 * len)) & 31u);
            if (code - c < first) {        // index + (code - first) < index + c <= k <= 19
                sym = vsb_sym5(s0, s1, index + (code - first));
                break;
            }
            index += c;
            first += c;
            first <<= 1;
            code <<= 1;
        }
        if (sym < 0) return false;
        vsi_drop(b, len);
        int rep = 1, val = sym;
        if (sym == 16) {
            if (idx == 0) return false;
            val = prev;
            rep = 3 + (int)vsi_take(b, 2);
        } else if (sym == 17) {
            val = 0;
            rep = 3 + (int)vsi_take(b, 3);
        } else if (sym == 18) {
            val = 0;
            rep = 11 + (int)vsi_take(b, 7);
        }
        if (b.err || idx + rep > total) return false;
        if (idx <= 256 && 256 < idx + rep) eob_len = val;
        if (val) {
            int nl = hlit - idx;           // how many of the run belong to the literal/length set
            nl = nl < 0 ? 0 : (nl > rep ? rep : nl);
            vsi_counter_add(lc, val, nl);
            vsi_counter_add(dc, val, rep - nl);
        }
        idx += rep;
        prev = val;
    }
    if (eob_len == 0) return false;
    int left = 1;
    for (int l = 1; l <= VSI_MAX_BITS; ++l) {
        left = 2 * left - vsi_counter_get(lc, l);
        if (left < 0) return false;
    }
    if (left != 0) return false;
    int maxlen = 0;
    left = 1;
    for (int l = 1; l <= VSI_MAX_BITS; ++l) {
        const int c = vsi_counter_get(dc, l);
        if (c) maxlen = l;
        left = 2 * left - c;
        if (left < 0) return false;
    }
    return left == 0 || maxlen <= 1;
}

// Whether `bit` is in the sorted list cand[0 .. n_cand).
VSI_HD bool vsb_is_candidate(const int64_t* cand, int64_t n_cand, int64_t bit) {
    int64_t lo = 0, hi = n_cand;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (cand[mid] < bit) lo = mid + 1; else hi = mid;
    }
    return lo < n_cand && cand[lo] == bit;
}

// ---- 1b. the finder of stored blocks (opt-in: vs_inflate_block_scan_stored) ------------------------------------------------------------
// A stored block's header is BFINAL, BTYPE = 00, zero bits up to the next byte boundary, then LEN and NLEN = ~LEN at that boundary.  Byte
// offset B is a STORED BOUNDARY when LEN and NLEN read there, complementary, and the LEN bytes behind them are followed by at least one
// more byte of the stream (a non-final block is followed by another header).  LEN = 0 counts: 00 00 ff ff is an empty stored block.
VSI_HD bool vsb_stored_boundary(const uint8_t* comp, int64_t n, int64_t B) {
    if (B < 0 || n < 4 || B > n - 4) return false;
    const uint32_t len = (uint32_t)comp[B] | ((uint32_t)comp[B + 1] << 8), nlen = (uint32_t)comp[B + 2] | ((uint32_t)comp[B + 3] << 8);
    return (len ^ 0xffffu) == nlen && B + 4 + (int64_t)len < n;
}

// How many bit positions in front of the stored boundary at bit 8 * B are candidates, given the 16 bits in front of it (bit 15 of `front`
// is stream bit 8 * B - 1; bits before the stream's first must be ones): the positions 8 * B - 3 - k, k = 0 .. count - 1, from each of
// which three header bits and k padding bits read as zeros.  0 .. 8.
VSI_HD int vsb_stored_count(uint32_t front) {
    const int zeros = __builtin_clz(((front & 0xffffu) << 16) | (1u << 21));   // zero bits straight in front of the boundary, 10 at most
    return zeros < 3 ? 0 : zeros - 2;
}

// Whether bit position `bit` of comp[0 .. n) is a candidate of the stored rule: the header bits BFINAL = 0, BTYPE = 00 read from it, at
// most seven zero bits pad it to a byte boundary, and that boundary is a stored boundary.  Reads bytes B - 2 .. B + 3 at most.
VSI_HD bool vsb_stored_start(const uint8_t* comp, int64_t n, int64_t bit) {
    if (bit < 0 || n < 4) return false;
    const int64_t B = (bit + 3 + 7) >> 3;                                   // the boundary behind the three header bits
    if (!vsb_stored_boundary(comp, n, B)) return false;
    for (int64_t q = bit; q < 8 * B; ++q)                                   // at most 10 bits, all in bytes B - 2 and B - 1
        if ((comp[q >> 3] >> (q & 7)) & 1u) return false;
    return true;
}

// ---- 2. a span -----------------------------------------------------------------------------------------------------------------------
// The probe's sink: a ring of VSB_WINDOW cells, appended to at pos (any number of bytes).  ext / reach are this lane's share.
struct VsbRing {
    uint16_t* cell;
    int64_t pos, ext;
    int reach, lane, nlanes;

    VSI_HD void lit(uint8_t v) {
        if (lane == 0) cell[pos & VSB_MASK] = v;
        ++pos;
    }
    VSI_HD uint16_t at(int64_t s) const { return s >= 0 ? cell[s & VSB_MASK] : (uint16_t)(VSC_EXT | (uint32_t)(-s - 1)); }
    VSI_HD void put(int64_t d, uint16_t c) {
        cell[d & VSB_MASK] = c;
        if (c & VSC_EXT) {
            ++ext;
            const int o1 = (int)(c & 0x7fffu) + 1;
            reach = o1 > reach ? o1 : reach;
        }
    }
    // 1 <= dist <= 32768, 3 <= len <= 258.  The cell a store replaces is 32768 behind it: no later read of this match wants it (a read is at
    // most `dist` behind its own store), and with dist = 32768 a lane reads the very cell it then rewrites with the same content.
    VSI_HD void copy(int dist, int len) {
        const int64_t sp = pos - dist;
        VSC_FENCE();
        if (dist >= nlanes) {                        // a turn reads only what earlier turns (or earlier tokens) wrote
            for (int j = 0; j < len; j += nlanes) {
                const int i = j + lane;
                if (i < len) put(pos + i, at(sp + i));
                VSC_FENCE();
            }
        } else {                                     // reads only what was there before the match
            for (int j = 0; j < len; j += nlanes) {
                const int i = j + lane;
                if (i < len) put(pos + i, at(sp + (int)((unsigned)i % (unsigned)dist)));
            }
            VSC_FENCE();                             // a later store of another lane to one of these cells (the ring comes round) is later
        }
        pos += len;
    }
    // len <= 65535: only the last VSB_WINDOW bytes have a cell of their own.  A long run comes round the ring to cells that other lanes wrote
    // just before it, and the next token to cells that other lanes write here: a fence on either side.
    VSI_HD void stored(const uint8_t* src, int len) {
        VSC_FENCE();
        for (int i = (len > VSB_WINDOW ? len - VSB_WINDOW : 0) + lane; i < len; i += nlanes) cell[(pos + i) & VSB_MASK] = src[i];
        VSC_FENCE();
        pos += len;
    }
};

// Blocks of comp[0 .. comp_bytes) from bit `start_bit` into `sink` (lit / copy / stored as above, int64 pos, lane, nlanes), as described at
// the head of this file.  r->status, end, final and produced are set (uniform); externals and reach are the caller's.
template <class Sink>
VSI_HD void vsb_inflate_span(const uint8_t* comp, int64_t comp_bytes, int64_t start_bit, const int64_t* cand, int64_t n_cand, int64_t stop_bit,
                             int64_t max_out, int64_t hist, VsiTables* t, Sink& sink, VscReport* r) {
    r->status = VS_INFLATE_INPUT; r->end = start_bit; r->final = 0; r->produced = 0; r->externals = 0; r->reach = 0;
    if (start_bit < 0 || comp_bytes < 0 || (start_bit >> 3) > comp_bytes) return;
    const int lane = sink.lane, nlanes = sink.nlanes;
    VsiBits b;
    b.in = comp;
    b.n = comp_bytes - (start_bit >> 3) < VSB_MAX_IN ? comp_bytes : (start_bit >> 3) + VSB_MAX_IN;
    b.pos = start_bit >> 3; b.buf = 0; b.cnt = 0; b.err = 0;
    vsi_take(b, (int)(start_bit & 7));
    int status = b.err;
    bool last = false, stop = false;
    while (!last && !stop && !status) {             // every turn consumes the three header bits or stops
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
            if (b.pos + (int64_t)len > b.n) { status = VS_INFLATE_INPUT; break; }
            if (sink.pos + (int64_t)len > max_out) { status = VS_INFLATE_OUT_LONG; break; }
            if (len) sink.stored(b.in + b.pos, (int)len);
            b.pos += len;
        } else {
            status = type == 1 ? vsi_fixed_tables(t, lane, nlanes) : vsi_dynamic_header(b, t, lane, nlanes);
            while (!status) {          // every turn consumes at least one bit or sets the status
                const int sym = vsi_decode(b, &t->lit);
                if (sym < 0) { status = b.err; break; }
                if (sym < 256) {
                    if (sink.pos >= max_out) { status = VS_INFLATE_OUT_LONG; break; }
                    sink.lit((uint8_t)sym);
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
                int dist = vsi_dist_base(ds);                               // at most 24577 + 8191 = 32768
                if (de > 8) {
                    dist += (int)vsi_take(b, 8);
                    dist += (int)vsi_take(b, de - 8) << 8;
                } else {
                    dist += (int)vsi_take(b, de);
                }
                if (b.err) { status = b.err; break; }
                if ((int64_t)dist > sink.pos + hist) { status = VS_INFLATE_DISTANCE; break; }
                if (sink.pos + len > max_out) { status = VS_INFLATE_OUT_LONG; break; }
                sink.copy(dist, len);
            }
        }
        if (!status && !last) {
            const int64_t at = b.pos * 8 - b.cnt;
            stop = cand ? vsb_is_candidate(cand, n_cand, at) : at >= stop_bit;
        }
    }
    if (status == VS_INFLATE_INPUT && b.n < comp_bytes) status = VS_INFLATE_CAP;   // not the stream ended, the span's allowance did
    r->status = status;
    r->final = (!status && last) ? 1 : 0;
    r->end = b.pos * 8 - b.cnt;
    r->produced = sink.pos;
}

// The probe of the candidate at `start_bit`: ring[0 .. VSB_WINDOW) is the wave's, every field of *r is set (uniform), and tail
// [0 .. min(produced, VSB_WINDOW)) receives the last cells in order.  Nothing else is written.
VSI_HD void vsb_probe(const uint8_t* comp, int64_t comp_bytes, int64_t start_bit, const int64_t* cand, int64_t n_cand, VsiTables* t, uint16_t* ring,
                      uint16_t* tail, VscReport* r, int lane, int nlanes) {
    VsbRing sink;
    sink.cell = ring; sink.pos = 0; sink.ext = 0; sink.reach = 0; sink.lane = lane; sink.nlanes = nlanes;
    vsb_inflate_span(comp, comp_bytes, start_bit, cand, n_cand, (int64_t)0, (int64_t)0x7fffffffffffffffll - 65536, (int64_t)VSB_WINDOW, t, sink, r);
    r->externals = VSB_WAVE_SUM64(sink.ext);
    r->reach = VSC_WAVE_MAX(sink.reach);
    VSC_FENCE();
    const int m = r->produced < VSB_WINDOW ? (int)r->produced : VSB_WINDOW;
    const int64_t from = r->produced - m;
    for (int i = lane; i < m; i += nlanes) tail[i] = ring[(from + i) & VSB_MASK];
}

// ---- 4. windows ----------------------------------------------------------------------------------------------------------------------
// Byte j of the window behind a span that produced `produced` bytes, from the window W before it and the span's tail cells.
VSI_HD uint8_t vsb_window_byte(const uint8_t* W, const uint16_t* tail, int64_t produced, int j) {
    const int m = produced < VSB_WINDOW ? (int)(produced < 0 ? 0 : produced) : VSB_WINDOW;
    if (j < VSB_WINDOW - m) return W[j + m];
    const uint32_t c = tail[j - (VSB_WINDOW - m)];
    return (c & VSC_EXT) ? W[VSB_WINDOW - 1 - (int)(c & 0x7fffu)] : (uint8_t)c;
}

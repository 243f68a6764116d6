// vs_deflate_window_core.h -- the logic of vs_deflate_chunks_window (csrc/vs_deflate.hip) as plain __host__ __device__ functions, on top of
// vs_deflate_core.h: the second matcher of the device encoder.  Where the RUNS matcher of vs_deflate_core.h knows literals and distance-1
// runs, the WINDOW matcher also finds a repeat up to 32768 bytes back -- the previous frame of a video-major array -- and may look for it
// BEFORE the chunk's first byte, in up to VSW_MAX_HISTORY bytes of `history`: bytes of the same array that a decoder of the concatenated
// stream has already produced.  The header compiles with a host compiler alone (tests/host/deflate_window_host_check.cpp): one logic, two
// builds, the kernel's bytes are the host's bytes.
//
// What one call makes: for ONE CHUNK (n <= VSD_MAX_CHUNK bytes at x, hist <= VSW_MAX_HISTORY bytes readable before x) one block + the sync
// marker, exactly as vsd_deflate_chunk does, and NEVER MORE BYTES than vsd_deflate_chunk makes of the same chunk:
//   1. the run-start mask of the chunk (as in vsd_deflate_chunk);
//   2. the search: per position of the chunk one (length, distance) into pk[] -- see vsw_match.  The candidate of a position is the last
//      earlier position with the same hash of 4 bytes in a table that is updated ONCE PER BLOCK OF 64 POSITIONS of history + chunk (all reads
//      of a block before all writes of it, the largest position wins).  The block of 64 is part of the definition, not of the launch;
//   3. vsd_deflate_chunk itself, into the image: the RUNS bytes and their exact bit count;
//   4. the greedy parse from position 0, next = i + length[i], as a bit per token start (in ww->mask), and the histograms of its tokens;
//   5. length-limited codes for literal/length (286 symbols) and distance (30 symbols, both 15 bits, vsd_build_lengths), the dynamic header
//      over hlit + hdist code lengths, the exact bits of the fixed and the dynamic form over this parse;
//   6. only if the smaller of the two is STRICTLY below the bits of the form vsd_deflate_chunk chose, the image is cleared and written
//      again from the window parse; otherwise the image stays what step 3 made: the RUNS bytes.  (Stored is the same under both parses.)
//
// Execution model: as vs_deflate_core.h -- `lane` of `nlanes` (host: 0 of 1; device: 0..63 of 64), the serial parts by lane 0 between
// VSD_SYNC()s.  Two more primitives with host defaults: VSW_TABLE_MAX (table[h] = max(table[h], p): lanes share the table) and VSW_CHAIN
// (which lanes of a window of nlanes positions the greedy chain visits, and where it leaves the window).  Every decision is a function of
// (history bytes, chunk bytes) only: a maximum does not depend on the order in which the lanes reach it, and the chain is defined by pk[].
//
// Termination and bounds, on ANY input (in addition to vs_deflate_core.h's):
//   * the search runs ceil((hist + n) / 64) blocks, hist + n <= 65536; per position the extension compares at most 258 bytes, 8 at a
//     time, and both sides of a comparison end at or before the chunk's last byte: the candidate lies before the position, and the
//     length is capped by n - i.  Nothing before x - hist is read: table entries are positions >= 0 of history + chunk (the table is
//     cleared per chunk, and an entry that was never written is position 0, verified like every other).  A match never extends past the
//     chunk's end and never starts before the first byte of history;
//   * the chain pass and the emission run ceil(n / nlanes) turns; the chain advances by at least 1 per token (pk holds lengths 1, 3..258
//     with i + length <= n), VSW_CHAIN doubles 6 times over a window of 64;
//   * pk[] holds n entries and is written for every position of the chunk before it is read; hdist <= 30 and hlit + hdist <= 316 entries
//     go through the header's run-length pass (cl_sym / cl_ext hold 320);
//   * a token is at most 15 + 5 + 15 + 13 = 48 bits and touches at most three words of the image; the window forms are only emitted when
//     their exact bit count is below that of the runs form, which is at most the stored form's, so they fit the image and the slot bound
//     n + VSD_SLOT_EXTRA.
// The image may overlap the HISTORY bytes (not the chunk's): history is not read after step 2.
#pragma once
#include "vs_deflate_core.h"

#ifndef VSW_TABLE_MAX
#define VSW_TABLE_MAX(p, v) (*(p) = *(p) < (v) ? (v) : *(p))
#define VSW_CHAIN(nx, entry, bits, out) ((bits) = 1ull, (out) = (nx))    /* a window of one position: entered at it, left for nx */
#endif

#define VSW_MAX_HISTORY VS_DEFLATE_MAX_HISTORY
#define VSW_HASH_BITS 14                            /* 64 KiB of table: an entry survives about 16384 entered positions */
#define VSW_DIST_SYMS 30
#define VSW_FAR 4096                                /* a length-3 match beyond this distance costs more than three literals */
#define VSW_FORM_RUNS (-1)                          /* s->form: the image is vsd_deflate_chunk's */

struct VswWork {
    uint32_t table[1 << VSW_HASH_BITS];             // hash of 4 bytes -> the last position (of history + chunk) of the blocks before
    uint32_t dfreq[VSW_DIST_SYMS];                  // distance histogram
    uint16_t dcode[VSW_DIST_SYMS];
    uint8_t dlen[VSW_DIST_SYMS];
    int32_t hdist, form, size, start_bit;           // form: VSW_FORM_RUNS, VSD_FORM_FIXED or VSD_FORM_DYNAMIC over the window parse
    int64_t bits[3];                                // exact bits of the window parse, [VSD_FORM_FIXED] and [VSD_FORM_DYNAMIC]
};

// Four bytes at ANY address, read as four bytes: the pointer is volatile so that the compiler does not merge them into one load of 4 or 8
// bytes, which for a position of a chunk in LDS is a wide DS load at an odd address.
VSD_HD uint32_t vsw_load4(const uint8_t* q) {
    const volatile uint8_t* p = q;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
VSD_HD uint64_t vsw_load8(const uint8_t* p) { return (uint64_t)vsw_load4(p) | ((uint64_t)vsw_load4(p + 4) << 32); }
VSD_HD uint32_t vsw_hash(uint32_t v) { return (v * 2654435761u) >> (32 - VSW_HASH_BITS); }

// distance - 1 (0..32767) -> symbol 0..29 and the number of its extra bits
VSD_HD int vsw_dist_sym(int d) {
    if (d < 4) return d;
    const int e = (31 - __builtin_clz((unsigned)d)) - 1;
    return 2 * e + 2 + ((d >> e) & 1);
}
VSD_HD int vsw_dist_extra(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }

// True when position p of y[0 .. P) takes part in the search: four bytes lie at it, and it is not the inside of a run of five equal bytes
// (there the distance-1 match of the mask is at least as long as any other, so such a position is neither looked up nor entered).
VSD_HD bool vsw_searched(const uint8_t* y, int P, int p) {
    if (p + 4 > P) return false;
    const uint32_t v = vsw_load4(y + p);
    return !(p >= 1 && v == (uint32_t)y[p] * 0x01010101u && y[p - 1] == y[p]);
}

// The token that would start at position i of the chunk, as length | (distance - 1) << 16: length 1 a literal, 3..258 a match.  The longer of
// the table's candidate (verified and extended; a length 3 beyond VSW_FAR dropped) and the distance-1 run of the mask; on a tie the run.
VSD_HD uint32_t vsw_match(const uint8_t* y, int hist, int n, int i, const uint64_t* mask, const uint32_t* table) {
    const int p = hist + i, maxlen = n - i < 258 ? n - i : 258;
    int rlen = 0;
    if (((mask[i >> 6] >> (i & 63)) & 1ull) == 0ull) rlen = vsd_next_set(mask, i + 1, i + maxlen) - i;
    if (rlen < 3) rlen = 0;
    if (rlen < maxlen && vsw_searched(y, hist + n, p)) {
        const int c = (int)table[vsw_hash(vsw_load4(y + p))];
        if (c < p && p - c <= 32768) {
            int m = 0;
            while (m + 8 <= maxlen) {               // at most 32 turns; c + m + 8 <= c + maxlen < p + maxlen <= hist + n
                const uint64_t d = vsw_load8(y + c + m) ^ vsw_load8(y + p + m);
                if (d) { m += __builtin_ctzll(d) >> 3; break; }
                m += 8;
            }
            if (m + 8 > maxlen)                     // fewer than 8 bytes are left (or the loop never ran): by bytes, at most 7 turns
                while (m < maxlen && y[c + m] == y[p + m]) ++m;
            if (m == 3 && p - c > VSW_FAR) m = 0;
            if (m >= 3 && m > rlen) return (uint32_t)m | ((uint32_t)(p - c - 1) << 16);
        }
    }
    return rlen ? (uint32_t)rlen : 1u;
}

// The run-length coded code lengths of a dynamic header over hlit literal/length and hdist distance lengths, as vsd_header_runs; lane 0.
VSD_HD void vsw_header_runs(VsdWork* w, const uint8_t* dlen, int hdist) {
    for (int i = 0; i < 19; ++i) w->cl_freq[i] = 0;
    int hlit = VSD_LIT_SYMS;
    while (hlit > 257 && w->len[hlit - 1] == 0) --hlit;
    w->hlit = hlit;
    const int total = hlit + hdist;
    int m = 0, i = 0;
    while (i < total) {                             // i advances by at least 1 per turn
        const int v = i < hlit ? w->len[i] : dlen[i - hlit];
        int run = 1;
        while (i + run < total && (i + run < hlit ? w->len[i + run] : dlen[i + run - hlit]) == v) ++run;
        i += run;
        if (v != 0) {
            w->cl_sym[m] = (uint8_t)v; w->cl_ext[m++] = 0; ++w->cl_freq[v];
            --run;
        }
        while (run >= 3) {
            const int r = v == 0 ? (run > 138 ? 138 : run) : (run > 6 ? 6 : run);
            const int sym = v != 0 ? 16 : (r <= 10 ? 17 : 18);
            w->cl_sym[m] = (uint8_t)sym; w->cl_ext[m++] = (uint8_t)(r - (sym == 18 ? 11 : 3)); ++w->cl_freq[sym];
            run -= r;
        }
        for (; run > 0; --run) { w->cl_sym[m] = (uint8_t)v; w->cl_ext[m++] = 0; ++w->cl_freq[v]; }
    }
    w->cl_n = m;
}

// One chunk: x[0 .. n), 0 <= n <= VSD_MAX_CHUNK, with x[-hist .. 0) readable, 0 <= hist <= VSW_MAX_HISTORY, into the image
// (vsd_image_words(n) words).  wr: the work of the runs parse (vsd_deflate_chunk's), ww: that of the window parse (ww->mask: the token
// starts), pk: n words.  Returns the chunk's bytes (uniform over the lanes); s->form tells whether the window parse was written.
VSD_HD int vsw_deflate_chunk(const uint8_t* x, int hist, int n, VsdWork* wr, VsdWork* ww, VswWork* s, uint32_t* pk, uint32_t* img, int lane,
                             int nlanes) {
    if (n == 0) {
        const int size = vsd_deflate_chunk(x, 0, wr, img, lane, nlanes);
        if (lane == 0) { s->form = VSW_FORM_RUNS; s->size = size; s->bits[1] = s->bits[2] = 0; }
        VSD_SYNC();
        return size;
    }
    const int mwords = (n >> 6) + 1, P = hist + n;
    const uint8_t* y = x - hist;
    VSD_SYNC();                                     // nobody still reads what the previous chunk left
    for (int i = lane; i < mwords; i += nlanes) { wr->mask[i] = 0ull; ww->mask[i] = 0ull; }
    for (int i = lane; i < (1 << VSW_HASH_BITS); i += nlanes) s->table[i] = 0u;
    for (int i = lane; i < VSD_MAX_SYMS; i += nlanes) ww->freq[i] = 0u;
    for (int i = lane; i < VSW_DIST_SYMS; i += nlanes) s->dfreq[i] = 0u;
    VSD_SYNC();
    // ---- 1. where runs start (as in vsd_deflate_chunk, which builds the same mask again in step 3) -------------------------------------
    for (int base = 0; base <= n; base += nlanes) {
        const int i = base + lane;
        const bool starts = i <= n && (i == 0 || i == n || x[i] != x[i - 1]);
        const uint64_t b = VSD_BALLOT(starts);
        if (lane == 0 && b) wr->mask[base >> 6] |= b << (base & 63);
    }
    // ---- 2. the search ---------------------------------------------------------------------------------------------------------------
    const int hb = hist & ~63;                      // the blocks that lie in the history altogether are only entered: a maximum, any order
    for (int p = lane; p < hb; p += nlanes)
        if (vsw_searched(y, P, p)) VSW_TABLE_MAX(&s->table[vsw_hash(vsw_load4(y + p))], (uint32_t)p);
    VSD_SYNC();
    for (int b = hb; b < P; b += 64) {
        for (int p = b + lane; p < b + 64 && p < P; p += nlanes)           // all reads of the block ...
            if (p >= hist) pk[p - hist] = vsw_match(y, hist, n, p - hist, wr->mask, s->table);
        VSD_SYNC();
        for (int p = b + lane; p < b + 64 && p < P; p += nlanes)           // ... before all its writes
            if (vsw_searched(y, P, p)) VSW_TABLE_MAX(&s->table[vsw_hash(vsw_load4(y + p))], (uint32_t)p);
        VSD_SYNC();
    }
    // ---- 3. the runs parse, complete: its bytes are in the image, its exact bits in wr->bits[wr->form] ----------------------------------
    const int runs_size = vsd_deflate_chunk(x, n, wr, img, lane, nlanes);
    // ---- 4. the greedy chain and the histograms of its tokens ------------------------------------------------------------------------
    int e = 0;                                      // where the next token starts
    for (int base = 0; base < n; base += nlanes) {
        if (e >= base + nlanes) continue;           // the window lies inside a match
        const int i = base + lane;
        const uint32_t t = i < n ? pk[i] : 1u;
        const int nx = i < n ? lane + (int)(t & 511u) : nlanes;
        uint64_t bits;
        int out;
        VSW_CHAIN(nx, e - base, bits, out);
        const bool starts = i < n && ((bits >> lane) & 1ull) != 0ull;
        const uint64_t b = VSD_BALLOT(starts);
        if (lane == 0 && b) ww->mask[base >> 6] |= b << (base & 63);
        if (starts) {
            const int len = (int)(t & 511u);
            if (len >= 3) {
                VSD_ATOMIC_ADD(&ww->freq[257 + vsd_len_index(len)], 1u);
                VSD_ATOMIC_ADD(&s->dfreq[vsw_dist_sym((int)(t >> 16))], 1u);
            } else {
                VSD_ATOMIC_ADD(&ww->freq[x[i]], 1u);
            }
        }
        e = base + out;
    }
    VSD_SYNC();
    if (lane == 0) ww->freq[VSD_EOB] = 1u;
    // ---- 5. the codes, the header, the exact bits, the choice ------------------------------------------------------------------------
    vsd_build_lengths(ww->freq, VSD_LIT_SYMS, 15, ww->len, ww->order, ww->a, lane, nlanes);
    vsd_build_lengths(s->dfreq, VSW_DIST_SYMS, 15, s->dlen, ww->order, ww->a, lane, nlanes);
    if (lane == 0) {
        int hdist = VSW_DIST_SYMS;
        while (hdist > 1 && s->dlen[hdist - 1] == 0) --hdist;                // no match: one code of zero bits
        s->hdist = hdist;
        vsw_header_runs(ww, s->dlen, hdist);
    }
    vsd_build_lengths(ww->cl_freq, 19, 7, ww->cl_len, ww->order, ww->a, lane, nlanes);
    if (lane == 0) {
        int64_t extra = 0, dyn = 0, fix = 0;
        for (int q = 0; q < VSD_LIT_SYMS; ++q) {
            const int64_t f = ww->freq[q];
            dyn += f * ww->len[q];
            fix += f * vsd_fixed_len(q);
            if (q > 256) extra += f * vsd_len_extra(q - 257);
        }
        for (int q = 0; q < VSW_DIST_SYMS; ++q) {
            const int64_t f = s->dfreq[q];
            dyn += f * (s->dlen[q] + vsw_dist_extra(q));
            fix += f * (5 + vsw_dist_extra(q));
        }
        int hclen = 19;
        while (hclen > 4 && ww->cl_len[vsd_cl_order(hclen - 1)] == 0) --hclen;
        ww->hclen = hclen;
        int64_t head = 3 + 5 + 5 + 4 + 3 * hclen;
        for (int k = 0; k < ww->cl_n; ++k) head += ww->cl_len[ww->cl_sym[k]] + vsd_cl_extra(ww->cl_sym[k]);
        s->bits[0] = wr->bits[wr->form];
        s->bits[VSD_FORM_FIXED] = 3 + fix + extra;
        s->bits[VSD_FORM_DYNAMIC] = head + dyn + extra;
        int form = VSW_FORM_RUNS;
        int64_t best = s->bits[0];
        if (s->bits[VSD_FORM_FIXED] < best) { form = VSD_FORM_FIXED; best = s->bits[VSD_FORM_FIXED]; }
        if (s->bits[VSD_FORM_DYNAMIC] < best) form = VSD_FORM_DYNAMIC;
        s->form = form;
        s->size = runs_size;
    }
    VSD_SYNC();
    const int form = s->form;
    if (form == VSW_FORM_RUNS) return runs_size;
    // ---- 6. the window parse into the image ----------------------------------------------------------------------------------------------
    const int words = vsd_image_words(n);
    for (int i = lane; i < words; i += nlanes) img[i] = 0u;
    VSD_SYNC();
    if (lane == 0) {
        int pos = 0;
        if (form == VSD_FORM_FIXED) {
            vsd_put(img, pos, 2u, 3);               // BFINAL 0, BTYPE 01
            for (int q = 0; q < VSD_MAX_SYMS; ++q) ww->len[q] = (uint8_t)vsd_fixed_len(q);
            vsd_assign_codes(ww->len, VSD_MAX_SYMS, ww->code);
            for (int q = 0; q < VSW_DIST_SYMS; ++q) s->dlen[q] = 5;
        } else {
            vsd_put(img, pos, 4u, 3);               // BFINAL 0, BTYPE 10
            vsd_put(img, pos, (uint32_t)(ww->hlit - 257), 5);
            vsd_put(img, pos, (uint32_t)(s->hdist - 1), 5);
            vsd_put(img, pos, (uint32_t)(ww->hclen - 4), 4);
            for (int k = 0; k < ww->hclen; ++k) vsd_put(img, pos, ww->cl_len[vsd_cl_order(k)], 3);
            vsd_assign_codes(ww->cl_len, 19, ww->cl_code);
            for (int k = 0; k < ww->cl_n; ++k) {
                const int sym = ww->cl_sym[k];
                vsd_put(img, pos, ww->cl_code[sym], ww->cl_len[sym]);
                vsd_put(img, pos, ww->cl_ext[k], vsd_cl_extra(sym));
            }
            vsd_assign_codes(ww->len, VSD_LIT_SYMS, ww->code);
        }
        vsd_assign_codes(s->dlen, VSW_DIST_SYMS, s->dcode);
        s->start_bit = pos;
    }
    VSD_SYNC();
    int pos = s->start_bit;
    for (int base = 0; base < n; base += nlanes) {
        const int i = base + lane;
        const bool starts = i < n && ((ww->mask[i >> 6] >> (i & 63)) & 1ull) != 0ull;
        if (VSD_BALLOT(starts) == 0ull) continue;   // no token starts in the window
        uint64_t v = 0;
        int nb = 0;
        if (starts) {
            const uint32_t t = pk[i];
            const int len = (int)(t & 511u);
            if (len >= 3) {
                const int idx = vsd_len_index(len), le = vsd_len_extra(idx), l = ww->len[257 + idx];
                const int d = (int)(t >> 16), ds = vsw_dist_sym(d), de = vsw_dist_extra(ds), dl = s->dlen[ds];
                v = (uint64_t)ww->code[257 + idx] | ((uint64_t)((len - 3) & ((1 << le) - 1)) << l);
                nb = l + le;
                v |= (uint64_t)s->dcode[ds] << nb;
                nb += dl;
                v |= (uint64_t)(d & ((1 << de) - 1)) << nb;
                nb += de;                           // at most 15 + 5 + 15 + 13 bits
            } else {
                v = ww->code[x[i]];
                nb = ww->len[x[i]];
            }
        }
        int before, total;
        VSD_SCAN(nb, before, total);
        const int at = pos + before;
        if (nb) {
            const int sh = at & 31;
            VSD_ATOMIC_OR(&img[at >> 5], (uint32_t)(v << sh));
            if (sh + nb > 32) VSD_ATOMIC_OR(&img[(at >> 5) + 1], (uint32_t)(v >> (32 - sh)));
            if (sh + nb > 64) VSD_ATOMIC_OR(&img[(at >> 5) + 2], (uint32_t)(v >> (64 - sh)));
        }
        pos += total;
    }
    VSD_SYNC();
    if (lane == 0) {
        vsd_put(img, pos, ww->code[VSD_EOB], ww->len[VSD_EOB]);
        pos = ((pos + 3 + 7) >> 3) << 3;            // the marker: 000, padding to a byte,
        vsd_put(img, pos, 0u, 16);                  // LEN = 0,
        vsd_put(img, pos, 0xFFFFu, 16);             // NLEN = 0xFFFF
        s->size = pos >> 3;
    }
    VSD_SYNC();
    return s->size;
}

// vs_deflate_core.h -- the logic of vs_deflate_chunks and vs_crc32 (csrc/vs_deflate.hip) as plain __host__ __device__ functions: the run
// finder, the tokens, the construction of length-limited Huffman codes, the exact cost of the three block forms of RFC 1951, the dynamic
// header and the emission of the bits; and the piecewise CRC-32 with its advance-by-zeros step.  The header compiles with a host compiler
// alone (tests/host/deflate_host_check.cpp), so the logic runs on the CPU, under sanitizers, before it runs on a GPU, and the kernel's
// bytes are the host's bytes: one logic, two builds.
//
// What one call makes: for ONE CHUNK of input (at most VSD_MAX_CHUNK bytes, independent of every other chunk) one complete block --
// stored, fixed or dynamic, whichever is smallest by its exact bit count -- followed by an empty stored block (00 00 FF FF after padding to
// a byte: the Z_SYNC_FLUSH form), so that chunks concatenate by bytes.  BFINAL is never set; the writer of the stream appends the final
// block.  An empty chunk is the marker alone.  Tokens are literals and (length 3..258, distance 1) matches: a run of R equal bytes is one
// literal and pieces of up to 258 bytes of the R - 1 that follow, a last piece of 1 or 2 bytes as literals.  There is no window search:
// on literal-heavy content this encoder is a Huffman coder.
//
// Execution model on the device: ONE WAVE PER CHUNK.  `lane` / `nlanes` (host: 0 of 1; device: 0..63 of 64) stripe the positions of the
// chunk over the lanes; the serial parts (code construction, the header) are done by lane 0 between VSD_SYNC()s.  The wave primitives are
// macros with host defaults: VSD_BALLOT (predicate -> bit per lane), VSD_SCAN (exclusive prefix sum and sum over the lanes),
// VSD_ATOMIC_ADD / VSD_ATOMIC_OR (on the histogram and the output image, which lanes share).  Every decision depends only on the chunk's
// bytes, never on nlanes.
//
// Termination and bounds, on ANY input:
//   * every loop over positions runs ceil(n / nlanes) turns, n <= VSD_MAX_CHUNK; vsd_next_set reads at most 6 words of the mask (it
//     looks at most 258 positions ahead); a skipped window advances the position by 64; the loops of the code builder run over at most
//     288 symbols (the rank sort 288 x 288), the Kraft repair at most VSD_MAX_SYMS turns, the header's run-length pass at most 316
//     entries; square-and-multiply of the CRC 64 x 32 steps;
//   * the output image holds vsd_image_words(n) words = the stored form + marker (n + 10 bytes) rounded up to a word; a fixed or dynamic
//     block is only emitted when its exact bit count is below the stored form's, so no form writes past the image, and the slot bound
//     n + VSD_SLOT_EXTRA is checked by the caller before the chunk is compressed;
//   * a match never reaches before the chunk's first byte: distance 1 from a position >= 1.
#pragma once
#include <stdint.h>

#include "../../include/varsep_hip.h"

#ifndef VSD_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define VSD_HD __host__ __device__ inline
#else
#define VSD_HD inline
#endif
#endif
#ifndef VSD_SYNC
#define VSD_SYNC() ((void)0)
#define VSD_BALLOT(p) ((uint64_t)((p) ? 1 : 0))
#define VSD_SCAN(v, before, total) ((before) = 0, (total) = (v))
#define VSD_ATOMIC_ADD(p, v) (*(p) += (v))
#define VSD_ATOMIC_OR(p, v) (*(p) |= (v))
#endif

#define VSD_MAX_CHUNK VS_DEFLATE_MAX_CHUNK          /* <= 65535: the stored form of a chunk is one block */
#define VSD_SLOT_EXTRA VS_DEFLATE_SLOT_EXTRA        /* 5 bytes of a stored block's header + 5 of the marker */
#define VSD_MAX_SYMS 288
#define VSD_LIT_SYMS 286
#define VSD_EOB 256
#define VSD_FORM_STORED 0
#define VSD_FORM_FIXED 1
#define VSD_FORM_DYNAMIC 2
#define VSD_FORM_EMPTY 3                            /* n == 0: the marker alone */

struct VsdWork {
    uint64_t mask[VSD_MAX_CHUNK / 64 + 1];          // bit i: position i starts a run (x[i] != x[i - 1], or i == 0); bit n: the sentinel
    uint32_t freq[VSD_MAX_SYMS];                    // literal/length histogram
    uint32_t a[VSD_MAX_SYMS];                       // scratch of the code builder
    uint16_t order[VSD_MAX_SYMS];                   // symbols by ascending (count, symbol)
    uint16_t code[VSD_MAX_SYMS];                    // bit-reversed canonical codes
    uint8_t len[VSD_MAX_SYMS];                      // code lengths, literal/length
    uint32_t cl_freq[19];
    uint16_t cl_code[19];
    uint8_t cl_len[19];
    uint8_t cl_sym[320], cl_ext[320];               // the header's code lengths, run-length coded: symbol and its extra bits' value
    int32_t cl_n, hlit, hclen;
    int32_t dist_len;                               // bits of the one distance code (distance 1): 0 without a match, 1 dynamic, 5 fixed
    int32_t form, size, start_bit;                  // the chosen form, the chunk's bytes, the bit at which the tokens start
    int64_t bits[3];                                // exact bits of the data block as stored / fixed / dynamic
};

VSD_HD int vsd_image_words(int n) { return (n + VSD_SLOT_EXTRA + 3) / 4; }

VSD_HD int vsd_len_index(int len) {                 // 3..258 -> 0..28 (symbol 257 + index)
    if (len == 258) return 28;
    const int l = len - 3;
    if (l < 8) return l;
    const int e = (31 - __builtin_clz((unsigned)l)) - 2;
    return 4 * e + 4 + ((l >> e) & 3);
}
VSD_HD int vsd_len_extra(int idx) { return idx < 8 || idx == 28 ? 0 : (idx - 4) >> 2; }
VSD_HD int vsd_fixed_len(int s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

// the first set bit of the mask at or after `from`, or `limit` when there is none below it; from <= limit <= n
VSD_HD int vsd_next_set(const uint64_t* mask, int from, int limit) {
    int wi = from >> 6;
    const int wl = limit >> 6;
    uint64_t word = mask[wi] & (~0ull << (from & 63));
    while (word == 0 && wi < wl) word = mask[++wi];  // at most (258 + 63) / 64 + 1 turns: limit <= from + 258
    if (word == 0) return limit;
    const int p = (wi << 6) + __builtin_ctzll(word);
    return p < limit ? p : limit;
}

// the start of the run position base + lane lies in: the last set bit at or below it (`carry`: the last set bit below base)
VSD_HD int vsd_run_start(const uint64_t* mask, int base, int lane, int carry) {
    const uint64_t word = mask[base >> 6] >> (base & 63);
    const uint64_t m = word & (lane >= 63 ? ~0ull : ((2ull << lane) - 1ull));
    return m ? base + 63 - __builtin_clzll(m) : carry;
}

// The token that STARTS at position i of a run that starts at s <= i: -1 none (inside a match), 0..255 a literal, 256 + length a match.
VSD_HD int vsd_token(const uint8_t* x, const uint64_t* mask, int n, int i, int s) {
    if (i == s) return x[i];
    const int o = (i - s - 1) % 258;                // offset inside the piece of up to 258 bytes
    const int ps = i - o;                           // where the piece starts: bits (s, i] of the mask are clear
    int lim = ps + 258;
    if (lim > n) lim = n;
    const int plen = vsd_next_set(mask, i + 1, lim) - ps;
    if (plen >= 3) return o == 0 ? 256 + plen : -1;
    return x[i];
}

// True when no token starts in the 64 positions from `base` (a multiple of 64): no run starts there (the mask word is clear, so the run that
// started at `carry` covers them and n >= base + 64), no piece of 258 starts there, and the run does not end within two positions behind
// them (a last piece of 1 or 2 bytes is literals).  Such a window -- background -- is skipped by both passes over the positions.
VSD_HD bool vsd_window_idle(const uint64_t* mask, int base, int carry) {
    if (mask[base >> 6] != 0ull || (mask[(base >> 6) + 1] & 3ull) != 0ull) return false;
    const int o = (base - carry - 1) % 258;         // base > carry: bit `base` is clear
    return o != 0 && o + 63 < 258;                  // offsets o .. o + 63 inside one piece, none of them its start
}

// Code lengths of at most max_bits for the symbols with freq > 0 (0 for the others), complete (Kraft sum exactly 1) when two or more
// symbols are used; a single used symbol gets one bit.  Moffat & Katajainen's in-place construction on the sorted counts, then the Kraft
// repair that takes one unit per turn.  order[], a[]: scratch of nsym entries.  Every lane calls it; lane 0 does the serial part.
VSD_HD void vsd_build_lengths(const uint32_t* freq, int nsym, int max_bits, uint8_t* len, uint16_t* order, uint32_t* a, int lane, int nlanes) {
    VSD_SYNC();
    for (int s = lane; s < nsym; s += nlanes) {     // rank sort: every used symbol finds its place
        const uint32_t f = freq[s];
        len[s] = 0;
        if (f == 0) continue;
        int rank = 0;
        for (int t = 0; t < nsym; ++t) {
            const uint32_t g = freq[t];
            rank += (g != 0 && (g < f || (g == f && t < s))) ? 1 : 0;
        }
        order[rank] = (uint16_t)s;
    }
    VSD_SYNC();
    if (lane == 0) {
        int n = 0;
        for (int s = 0; s < nsym; ++s) n += freq[s] != 0 ? 1 : 0;
        if (n == 1) len[order[0]] = 1;
        if (n >= 2) {
            for (int k = 0; k < n; ++k) a[k] = freq[order[k]];
            a[0] += a[1];
            int root = 0, leaf = 2;
            for (int next = 1; next < n - 1; ++next) {
                if (leaf >= n || a[root] < a[leaf]) { a[next] = a[root]; a[root++] = (uint32_t)next; }
                else a[next] = a[leaf++];
                if (leaf >= n || (root < next && a[root] < a[leaf])) { a[next] += a[root]; a[root++] = (uint32_t)next; }
                else a[next] += a[leaf++];
            }
            a[n - 2] = 0;
            for (int next = n - 3; next >= 0; --next) a[next] = a[a[next]] + 1;
            int avbl = 1, used = 0, dpth = 0, next = n - 1;
            root = n - 2;
            while (avbl > 0) {                      // one turn per depth; depth < n
                while (root >= 0 && (int)a[root] == dpth) { ++used; --root; }
                while (avbl > used) { a[next--] = (uint32_t)dpth; --avbl; }
                avbl = 2 * used;
                ++dpth;
                used = 0;
            }
            // a[k]: the depth of the k-th symbol by ascending count, non-increasing in k
            int count[16];
            for (int b = 0; b < 16; ++b) count[b] = 0;
            for (int k = 0; k < n; ++k) ++count[(int)a[k] > max_bits ? max_bits : (int)a[k]];
            uint32_t total = 0;
            for (int b = 1; b <= max_bits; ++b) total += (uint32_t)count[b] << (max_bits - b);
            for (int turn = 0; turn < VSD_MAX_SYMS && total > (1u << max_bits); ++turn) {
                --count[max_bits];                  // one leaf leaves the deepest level and becomes the sibling of a leaf moved one level down
                for (int b = max_bits - 1; b > 0; --b)
                    if (count[b]) { --count[b]; count[b + 1] += 2; break; }
                --total;
            }
            int k = 0;
            for (int b = max_bits; b >= 1; --b)
                for (int c = 0; c < count[b]; ++c) len[order[k++]] = (uint8_t)b;
        }
    }
    VSD_SYNC();
}

// bit-reversed canonical codes of lengths len[0 .. nsym); lane 0 only
VSD_HD void vsd_assign_codes(const uint8_t* len, int nsym, uint16_t* code) {
    int count[16], next[16];
    for (int b = 0; b < 16; ++b) count[b] = 0;
    for (int s = 0; s < nsym; ++s) ++count[len[s] & 15];
    count[0] = 0;
    int c = 0;
    next[0] = 0;
    for (int b = 1; b < 16; ++b) {
        c = (c + count[b - 1]) << 1;
        next[b] = c;
    }
    for (int s = 0; s < nsym; ++s) {
        const int l = len[s] & 15;
        uint32_t v = l ? (uint32_t)next[l]++ : 0u, r = 0;
        for (int b = 0; b < l; ++b) { r = (r << 1) | (v & 1u); v >>= 1; }
        code[s] = (uint16_t)r;
    }
}

// nb <= 32 bits of v at bit `pos` of the image (plain read-modify-write: one lane, between two VSD_SYNC()s)
VSD_HD void vsd_put(uint32_t* img, int& pos, uint32_t v, int nb) {
    if (nb == 0) return;
    const int sh = pos & 31;
    img[pos >> 5] |= v << sh;
    if (sh + nb > 32) img[(pos >> 5) + 1] |= v >> (32 - sh);
    pos += nb;
}

// The run-length coded code lengths of a dynamic header (RFC 1951 3.2.7) into w->cl_sym / cl_ext and their histogram; lane 0 only.
VSD_HD void vsd_header_runs(VsdWork* w) {
    for (int i = 0; i < 19; ++i) w->cl_freq[i] = 0;
    int hlit = VSD_LIT_SYMS;
    while (hlit > 257 && w->len[hlit - 1] == 0) --hlit;
    w->hlit = hlit;
    const int total = hlit + 1;                     // HDIST = 1: the one distance code, of dist_len bits
    int m = 0, i = 0;
    while (i < total) {                             // i advances by at least 1 per turn
        const int v = i < hlit ? w->len[i] : (w->dist_len ? 1 : 0);
        int run = 1;
        while (i + run < total && (i + run < hlit ? w->len[i + run] : (w->dist_len ? 1 : 0)) == v) ++run;
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

VSD_HD int vsd_cl_order(int i) {
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}
VSD_HD int vsd_cl_extra(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }

// One chunk: x[0 .. n), 0 <= n <= VSD_MAX_CHUNK, into the image (vsd_image_words(n) words; readable by every lane after the call).
// Returns the chunk's bytes (uniform over the lanes); w->form and w->bits tell what was chosen and why.
VSD_HD int vsd_deflate_chunk(const uint8_t* x, int n, VsdWork* w, uint32_t* img, int lane, int nlanes) {
    const int words = vsd_image_words(n), mwords = (n >> 6) + 1;
    VSD_SYNC();                                     // nobody still reads what the previous chunk left
    for (int i = lane; i < words; i += nlanes) img[i] = 0u;
    for (int i = lane; i < mwords; i += nlanes) w->mask[i] = 0ull;
    for (int i = lane; i < VSD_MAX_SYMS; i += nlanes) w->freq[i] = 0u;
    VSD_SYNC();
    if (n == 0) {
        if (lane == 0) {
            int pos = 8;                            // 000 + padding, then LEN = 0, NLEN = 0xFFFF
            vsd_put(img, pos, 0u, 16);
            vsd_put(img, pos, 0xFFFFu, 16);
            w->form = VSD_FORM_EMPTY; w->size = 5;
            w->bits[0] = w->bits[1] = w->bits[2] = 0;
        }
        VSD_SYNC();
        return 5;
    }
    // ---- where runs start -------------------------------------------------------------------------------------------------------
    for (int base = 0; base <= n; base += nlanes) { // position n is the sentinel
        const int i = base + lane;
        const bool starts = i <= n && (i == 0 || i == n || x[i] != x[i - 1]);
        const uint64_t b = VSD_BALLOT(starts);
        if (lane == 0 && b) w->mask[base >> 6] |= b << (base & 63);
    }
    VSD_SYNC();
    // ---- the histogram of the tokens --------------------------------------------------------------------------------------------
    int carry = 0;
    for (int base = 0; base < n; base += nlanes) {
        if ((base & 63) == 0 && vsd_window_idle(w->mask, base, carry)) {
            base += 64 - nlanes;
            continue;
        }
        const int i = base + lane;
        if (i < n) {
            const int t = vsd_token(x, w->mask, n, i, vsd_run_start(w->mask, base, lane, carry));
            if (t >= 0) VSD_ATOMIC_ADD(&w->freq[t < 256 ? t : 257 + vsd_len_index(t - 256)], 1u);
        }
        carry = vsd_run_start(w->mask, base, nlanes - 1, carry);
    }
    if (lane == 0) w->freq[VSD_EOB] = 1u;
    vsd_build_lengths(w->freq, VSD_LIT_SYMS, 15, w->len, w->order, w->a, lane, nlanes);
    // ---- the three forms' exact bits, the choice, the header ----------------------------------------------------------------------
    if (lane == 0) {
        uint32_t matches = 0;
        for (int s = 257; s < VSD_LIT_SYMS; ++s) matches += w->freq[s];
        w->dist_len = matches ? 1 : 0;              // no match: one distance code of zero bits
        vsd_header_runs(w);
    }
    vsd_build_lengths(w->cl_freq, 19, 7, w->cl_len, w->order, w->a, lane, nlanes);
    if (lane == 0) {
        int64_t extra = 0, matches = 0, dyn = 0, fix = 0;
        for (int s = 0; s < VSD_LIT_SYMS; ++s) {
            const int64_t f = w->freq[s];
            dyn += f * w->len[s];
            fix += f * vsd_fixed_len(s);
            if (s > 256) { matches += f; extra += f * vsd_len_extra(s - 257); }
        }
        int hclen = 19;
        while (hclen > 4 && w->cl_len[vsd_cl_order(hclen - 1)] == 0) --hclen;
        w->hclen = hclen;
        int64_t head = 3 + 5 + 5 + 4 + 3 * hclen;
        for (int k = 0; k < w->cl_n; ++k) head += w->cl_len[w->cl_sym[k]] + vsd_cl_extra(w->cl_sym[k]);
        w->bits[VSD_FORM_STORED] = 8 * (int64_t)(5 + n);
        w->bits[VSD_FORM_FIXED] = 3 + fix + extra + 5 * matches;
        w->bits[VSD_FORM_DYNAMIC] = head + dyn + extra + matches;
        int form = VSD_FORM_STORED;
        if (w->bits[VSD_FORM_FIXED] < w->bits[form]) form = VSD_FORM_FIXED;
        if (w->bits[VSD_FORM_DYNAMIC] < w->bits[form]) form = VSD_FORM_DYNAMIC;
        w->form = form;
        int pos = 0;
        if (form == VSD_FORM_STORED) {
            pos = 8;                                // BFINAL 0, BTYPE 00, padding
            vsd_put(img, pos, (uint32_t)n, 16);
            vsd_put(img, pos, (uint32_t)n ^ 0xFFFFu, 16);
        } else if (form == VSD_FORM_FIXED) {
            vsd_put(img, pos, 2u, 3);               // BFINAL 0, BTYPE 01
            for (int s = 0; s < VSD_LIT_SYMS; ++s) w->len[s] = (uint8_t)vsd_fixed_len(s);
            for (int s = VSD_LIT_SYMS; s < VSD_MAX_SYMS; ++s) w->len[s] = 8;
            vsd_assign_codes(w->len, VSD_MAX_SYMS, w->code);
            w->dist_len = matches ? 5 : 0;
        } else {
            vsd_put(img, pos, 4u, 3);               // BFINAL 0, BTYPE 10
            vsd_put(img, pos, (uint32_t)(w->hlit - 257), 5);
            vsd_put(img, pos, 0u, 5);               // HDIST - 1
            vsd_put(img, pos, (uint32_t)(hclen - 4), 4);
            for (int k = 0; k < hclen; ++k) vsd_put(img, pos, w->cl_len[vsd_cl_order(k)], 3);
            vsd_assign_codes(w->cl_len, 19, w->cl_code);
            for (int k = 0; k < w->cl_n; ++k) {
                const int sym = w->cl_sym[k];
                vsd_put(img, pos, w->cl_code[sym], w->cl_len[sym]);
                vsd_put(img, pos, w->cl_ext[k], vsd_cl_extra(sym));
            }
            vsd_assign_codes(w->len, VSD_LIT_SYMS, w->code);
        }
        w->start_bit = pos;
    }
    VSD_SYNC();
    const int form = w->form;
    int pos = w->start_bit;
    if (form == VSD_FORM_STORED) {
        uint8_t* bytes = reinterpret_cast<uint8_t*>(img) + 5;
        for (int i = lane; i < n; i += nlanes) bytes[i] = x[i];
        pos += 8 * n;
    } else {
        const int dist_len = w->dist_len;
        carry = 0;
        for (int base = 0; base < n; base += nlanes) {
            if ((base & 63) == 0 && vsd_window_idle(w->mask, base, carry)) {
                base += 64 - nlanes;
                continue;
            }
            const int i = base + lane;
            uint32_t v = 0;
            int nb = 0;
            if (i < n) {
                const int t = vsd_token(x, w->mask, n, i, vsd_run_start(w->mask, base, lane, carry));
                if (t >= 256) {
                    const int idx = vsd_len_index(t - 256), e = vsd_len_extra(idx), l = w->len[257 + idx];
                    v = (uint32_t)w->code[257 + idx] | ((uint32_t)((t - 259) & ((1 << e) - 1)) << l);
                    nb = l + e + dist_len;          // the distance code of distance 1 is all zeros, and 258 has no extra bits: (258 - 3) & 0
                } else if (t >= 0) {
                    v = w->code[t];
                    nb = w->len[t];
                }
            }
            int before, total;
            VSD_SCAN(nb, before, total);
            const int at = pos + before;
            if (nb) {
                const int sh = at & 31;
                VSD_ATOMIC_OR(&img[at >> 5], v << sh);
                if (sh + nb > 32) VSD_ATOMIC_OR(&img[(at >> 5) + 1], v >> (32 - sh));
            }
            pos += total;
            carry = vsd_run_start(w->mask, base, nlanes - 1, carry);
        }
    }
    VSD_SYNC();
    if (lane == 0) {
        if (form != VSD_FORM_STORED) vsd_put(img, pos, w->code[VSD_EOB], w->len[VSD_EOB]);
        pos = ((pos + 3 + 7) >> 3) << 3;            // the marker: 000, padding to a byte,
        vsd_put(img, pos, 0u, 16);                  // LEN = 0,
        vsd_put(img, pos, 0xFFFFu, 16);             // NLEN = 0xFFFF
        w->size = pos >> 3;
    }
    VSD_SYNC();
    return w->size;
}

// ---- CRC-32 (the zip polynomial, reflected), piecewise ---------------------------------------------------------------------------
// The register after bytes D from state c is linear over GF(2): update(c, D) = update(c, zeros(|D|)) ^ update(0, D), and advancing a state
// past k zero bytes is a multiplication by x^(8k) mod P.  So zlib.crc32(data, init) = ~(shift(~init, n) ^ XOR over the pieces of
// shift(update(0, piece), bytes after the piece)), and every piece is independent.
#define VSD_CRC_POLY 0xEDB88320u

VSD_HD uint32_t vsd_crc_table_entry(uint32_t b) {
    for (int k = 0; k < 8; ++k) b = (b & 1u) ? (b >> 1) ^ VSD_CRC_POLY : b >> 1;
    return b;
}
VSD_HD uint32_t vsd_crc_bytes(const uint32_t* table, const uint8_t* p, int64_t n, uint32_t c) {
    int64_t i = 0;
    for (; i < n && ((uintptr_t)(p + i) & 3u) != 0; ++i) c = table[(c ^ p[i]) & 255u] ^ (c >> 8);
    for (; i + 4 <= n; i += 4) {                    // aligned words: one load per four bytes
        c ^= *reinterpret_cast<const uint32_t*>(__builtin_assume_aligned(p + i, 4));
        for (int k = 0; k < 4; ++k) c = table[c & 255u] ^ (c >> 8);
    }
    for (; i < n; ++i) c = table[(c ^ p[i]) & 255u] ^ (c >> 8);
    return c;
}
// a * b mod P, bit 31 = x^0 (32 steps)
VSD_HD uint32_t vsd_gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 31; k >= 0; --k) {
        p ^= ((a >> k) & 1u) ? b : 0u;
        b = (b & 1u) ? (b >> 1) ^ VSD_CRC_POLY : b >> 1;
    }
    return p;
}
// the state c advanced past nbytes >= 0 zero bytes: c * x^(8 nbytes) mod P, square-and-multiply over the at most 64 bits of the exponent
VSD_HD uint32_t vsd_crc_shift(uint32_t c, int64_t nbytes) {
    if (c == 0u) return 0u;
    uint64_t e = (uint64_t)nbytes;
    uint32_t sq = vsd_gf_mul(vsd_gf_mul(0x40000000u, 0x40000000u), vsd_gf_mul(0x40000000u, 0x40000000u));   // x^4
    sq = vsd_gf_mul(sq, sq);                        // x^8: one byte
    for (int k = 0; k < 64 && e; ++k, e >>= 1) {
        if (e & 1u) c = vsd_gf_mul(c, sq);
        sq = vsd_gf_mul(sq, sq);
    }
    return c;
}
// lane's share of the piece [lo, hi) of an array of n bytes (`piece` points at byte lo): the lanes' results XOR to the piece's partial.
// The piece is cut into nlanes sub-pieces of a multiple of 4 bytes; the piece that starts at 0 carries the term of the initial state.
VSD_HD uint32_t vsd_crc_partial(const uint32_t* table, const uint8_t* piece, int64_t n, int64_t lo, int64_t hi, uint32_t init, int lane,
                                int nlanes) {
    const int64_t len = hi - lo, sub = ((len + nlanes - 1) / nlanes + 3) & ~(int64_t)3;
    int64_t a = sub * lane, b = a + sub;
    if (a > len) a = len;
    if (b > len) b = len;
    uint32_t r = vsd_crc_shift(vsd_crc_bytes(table, piece + a, b - a, 0u), n - lo - b);
    if (lo == 0 && lane == 0) r ^= vsd_crc_shift(~init, n);
    return r;
}

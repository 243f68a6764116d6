// vs_inflate_chunks_core.h -- the logic of vs_inflate_segments (csrc/vs_inflate_chunks.hip) as plain __host__ __device__ functions on top of
// csrc/vs_inflate_core.h: the decode of ONE SEGMENT of a raw RFC 1951 stream that starts at a byte offset and does not know what came before
// it.  Every stream this project writes is cut at byte-aligned empty stored blocks (00 00 FF FF): the byte after such a marker is where a
// segment may start, and a decoder that starts one segment per marker decodes a member of any size in parallel.  The header compiles with a
// host compiler alone (tests/host/inflate_chunks_host_check.cpp runs it under sanitizers on valid, on speculative and on damaged input).
//
// A segment: blocks (stored, fixed, dynamic) are decoded from `start` until
//   * an empty stored block (LEN = 0) has been consumed: `end` is the byte after it (the marker: its last four bytes are 00 00 FF FF);
//   * a block with BFINAL = 1 has ended: `final` is set and `end` is the next byte boundary;
//   * an error: `status` is a VS_INFLATE_* code (VS_INFLATE_OUT_LONG for more than VSC_MAX_OUT bytes of output, VS_INFLATE_INPUT for a
//     segment that is not over after VSC_MAX_IN bytes of input or at the end of the stream).
// What is before the segment is unknown, so a match whose source lies before the segment's first byte is no error: such a byte is EXTERNAL and
// records o in 0..32767, its source being the byte start_of_output - 1 - o of the member; a byte copied from an external byte inherits the
// record.  The output lives in CELLS of 16 bits, one per byte: the value, or VSC_EXT | o.  After the decode every cell is a value or a
// reference to a position strictly before the segment, which vs_inflate_resolve fills in chain order.
//
// Execution model as in vs_inflate_core.h: one wave per segment, every lane runs this code with the same values; `lane` / `nlanes` stripe the
// copies and the final count over the lanes (the host passes lane 0 of 1).  VSC_FENCE() orders a phase that writes cells before one that
// reads them (a wave-scope fence on the device), VSC_WAVE_SUM / VSC_WAVE_MAX combine the lanes' partial results.
//
// Termination and bounds, on ANY input (speculative starts feed garbage on purpose):
//   * the bit reader is vs_inflate_core.h's, over [comp + start, comp + start + min(comp_bytes - start, VSC_MAX_IN)): nothing outside the
//     stream is read, and a segment reads at most VSC_MAX_IN bytes however the bits go (a chain of empty blocks produces nothing and would
//     otherwise run to the end of a member of any size);
//   * the block loop consumes the three header bits per turn or stops, the symbol loop one bit per turn or stops, as there; tables are
//     validated before they are built, symbols are range-checked before they index a table;
//   * a cell is written only at pos + i < pos + len <= VSC_MAX_OUT (checked before every literal, match and stored run), and a copy reads
//     cell[s] only for 0 <= s < pos; for s < 0 it reads nothing and forms VSC_EXT | (-s - 1), where -s - 1 <= 32767 because a distance is at
//     most 32768 (distance symbols above 29 are refused).
#pragma once
#include "vs_inflate_core.h"

#ifndef VSC_FENCE
#define VSC_FENCE() ((void)0)
#endif
#ifndef VSC_WAVE_SUM
#define VSC_WAVE_SUM(v) (v)
#define VSC_WAVE_MAX(v) (v)
#endif

#define VSC_MAX_OUT VS_DEFLATE_MAX_CHUNK            /* bytes a segment may produce */
#define VSC_MAX_IN (2 * VS_DEFLATE_MAX_CHUNK)       /* bytes a segment may read */
#define VSC_EXT 0x8000u                             /* cell: an external byte, o in the low 15 bits */

// What a segment reports (the VS_INFLATE_REPORT_WORDS int64 words of vs_inflate_segments, in this order).
struct VscReport {
    int64_t status, end, final, produced, externals, reach;   // reach: the largest o + 1 (0 without externals)
};

// The sink of a segment: cell[0 .. VSC_MAX_OUT), appended to at pos.
struct VscCells {
    uint16_t* cell;
    int pos, lane, nlanes;

    VSI_HD void lit(uint8_t v) {
        if (lane == 0) cell[pos] = v;
        ++pos;
    }
    VSI_HD uint16_t at(int s) const { return s >= 0 ? cell[s] : (uint16_t)(VSC_EXT | (uint32_t)(-s - 1)); }
    VSI_HD void copy(int dist, int len) {            // 1 <= dist <= 32768, 3 <= len <= 258, pos + len <= VSC_MAX_OUT
        const int sp = pos - dist;                   // >= -32768
        VSC_FENCE();
        if (dist >= nlanes) {                        // a turn reads only what earlier turns (or earlier tokens) wrote
            for (int j = 0; j < len; j += nlanes) {
                const int i = j + lane;
                if (i < len) cell[pos + i] = at(sp + i);
                VSC_FENCE();
            }
        } else {                                     // reads only what was there before the match
            for (int j = 0; j < len; j += nlanes) {
                const int i = j + lane;
                if (i < len) cell[pos + i] = at(sp + (int)((unsigned)i % (unsigned)dist));
            }
        }
        pos += len;
    }
    VSI_HD void stored(const uint8_t* src, int len) {   // pos + len <= VSC_MAX_OUT
        for (int i = lane; i < len; i += nlanes) cell[pos + i] = src[i];
        pos += len;
    }
};

// One segment of the raw stream comp[0 .. comp_bytes) from byte `start` into cell[0 .. VSC_MAX_OUT).  Every field of *r is set (uniform).
VSI_HD void vsc_inflate_segment(const uint8_t* comp, int64_t comp_bytes, int64_t start, VsiTables* t, uint16_t* cell, VscReport* r, int lane,
                                int nlanes) {
    r->status = VS_INFLATE_INPUT; r->end = start; r->final = 0; r->produced = 0; r->externals = 0; r->reach = 0;
    if (start < 0 || start > comp_bytes) return;
    VsiBits b;
    b.in = comp + start;
    b.n = comp_bytes - start < VSC_MAX_IN ? comp_bytes - start : VSC_MAX_IN;
    b.pos = 0; b.buf = 0; b.cnt = 0; b.err = 0;
    VscCells sink;
    sink.cell = cell; sink.pos = 0; sink.lane = lane; sink.nlanes = nlanes;
    int status = 0;
    bool last = false, marker = false;
    while (!last && !marker && !status) {           // every turn consumes the three header bits or stops
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
            if (len == 0) { marker = true; break; }
            if (b.pos + (int64_t)len > b.n) { status = VS_INFLATE_INPUT; break; }
            if (sink.pos + (int)len > VSC_MAX_OUT) { status = VS_INFLATE_OUT_LONG; break; }
            sink.stored(b.in + b.pos, (int)len);
            b.pos += len;
            continue;
        }
        status = type == 1 ? vsi_fixed_tables(t, lane, nlanes) : vsi_dynamic_header(b, t, lane, nlanes);
        while (!status) {              // every turn consumes at least one bit or sets the status
            const int sym = vsi_decode(b, &t->lit);
            if (sym < 0) { status = b.err; break; }
            if (sym < 256) {
                if (sink.pos >= VSC_MAX_OUT) { status = VS_INFLATE_OUT_LONG; break; }
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
            int dist = vsi_dist_base(ds);                                   // at most 24577 + 8191 = 32768
            if (de > 8) {
                dist += (int)vsi_take(b, 8);
                dist += (int)vsi_take(b, de - 8) << 8;
            } else {
                dist += (int)vsi_take(b, de);
            }
            if (b.err) { status = b.err; break; }
            if (sink.pos + len > VSC_MAX_OUT) { status = VS_INFLATE_OUT_LONG; break; }
            sink.copy(dist, len);                                           // a source before the segment is external, not an error
        }
    }
    if (!status && !marker) vsi_drop(b, b.cnt & 7);                         // a final block: to the next byte boundary
    r->status = status;
    r->final = (!status && last) ? 1 : 0;
    r->end = start + b.pos - (b.cnt >> 3);
    r->produced = sink.pos;
    VSC_FENCE();
    int externals = 0, reach = 0;
    for (int i = lane; i < sink.pos; i += nlanes) {
        const uint32_t c = cell[i];
        if (c & VSC_EXT) {
            ++externals;
            const int o1 = (int)(c & 0x7fffu) + 1;
            reach = o1 > reach ? o1 : reach;
        }
    }
    r->externals = VSC_WAVE_SUM(externals);
    r->reach = VSC_WAVE_MAX(reach);
}

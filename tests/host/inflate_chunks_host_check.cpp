// Host check of csrc/vs_inflate_chunks_core.h: the segment decoder of vs_inflate_segments, compiled for the CPU (with sanitizers where
// they link) and run on a case file that tests/inflate_chunks_inputs.py writes.  Per record the program does what the device route does:
// the scan for 00 00 FF FF, one segment decode per candidate, the chain walk from offset 0, the placing of the chain's segments and the
// filling of their external bytes in chain order -- and compares the result with the bytes zlib produced.  The input, the cells and the
// output are exactly-sized heap buffers (a read or a write outside them is a sanitizer report); the cells and the output also carry guard
// bytes on both sides, which are checked after every decode.
//
//   inflate_chunks_host_check CASES OUT
// CASES (little-endian): int64 records; per record int64 comp_bytes, int64 out_bytes, int64 mode, the stream, the bytes zlib produced.
// mode 1: the stream is also decoded from offset 0 truncated at every byte, and from every candidate with 200 single-byte corruptions
// (seeded): every such decode must end with a status and a sane report.
// OUT: int64 records; per record int64 n_cand, int64 chain_ok, int64 chain_len, int64 produced, cand [n_cand], words [n_cand * 6], chain
// (candidate indices) [chain_len], the output [produced] (produced = 0 unless chain_ok).
// Prints one line per mismatch and a summary line; the exit status is 0 unless a file cannot be read or written.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../spatiotemporal_variable_separation_amd/csrc/vs_inflate_chunks_core.h"

static const int GUARD = 64;

static int read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static int write_exact(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }

static long mismatches = 0, decodes = 0;

struct Cells {
    uint16_t* all;
    uint16_t* cell;
    Cells() {
        all = (uint16_t*)malloc((size_t)(VSC_MAX_OUT + 2 * GUARD) * 2);
        cell = all + GUARD;
    }
    ~Cells() { free(all); }
    void arm() {
        for (int i = 0; i < GUARD; ++i) all[i] = all[GUARD + VSC_MAX_OUT + i] = 0xA5A5;
        memset(cell, 0x5A, (size_t)VSC_MAX_OUT * 2);           // nothing may depend on what a previous segment left
    }
    bool intact() const {
        for (int i = 0; i < GUARD; ++i)
            if (all[i] != 0xA5A5 || all[GUARD + VSC_MAX_OUT + i] != 0xA5A5) return false;
        return true;
    }
};

// One decode from an exactly-sized heap copy of comp[0 .. n); the report must be sane whatever the bytes are.
static void decode(const uint8_t* comp, int64_t n, int64_t start, VsiTables* t, Cells& cells, VscReport* r, const char* what, long long tag) {
    uint8_t* in = (uint8_t*)malloc(n ? (size_t)n : 1);
    memcpy(in, comp, (size_t)n);
    memset(t, 0xA5, sizeof(VsiTables));
    cells.arm();
    vsc_inflate_segment(in, n, start, t, cells.cell, r, 0, 1);
    free(in);
    ++decodes;
    const bool sane = r->status >= 0 && r->status <= 10 && r->produced >= 0 && r->produced <= VSC_MAX_OUT && r->end >= start && r->end <= n &&
                      r->end - start <= VSC_MAX_IN && (r->final == 0 || r->final == 1) && r->externals >= 0 && r->externals <= r->produced &&
                      r->reach >= 0 && r->reach <= 32768 && (r->externals > 0) == (r->reach > 0) && (r->final == 0 || r->status == 0);
    if (!sane || !cells.intact()) {
        ++mismatches;
        printf("%s %lld start %lld: report status %lld end %lld final %lld produced %lld externals %lld reach %lld, guards %s\n", what, tag, (long long)start,
               (long long)r->status, (long long)r->end, (long long)r->final, (long long)r->produced, (long long)r->externals, (long long)r->reach,
               cells.intact() ? "intact" : "OVERWRITTEN");
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    int64_t records = 0;
    if (!read_exact(f, &records, 8) || !write_exact(g, &records, 8)) return 2;
    VsiTables* tables = (VsiTables*)malloc(sizeof(VsiTables));
    Cells cells;
    long chained = 0, segments = 0;
    for (int64_t rec = 0; rec < records; ++rec) {
        int64_t head[3];
        if (!read_exact(f, head, sizeof(head))) return 2;
        const int64_t n = head[0], want_bytes = head[1], mode = head[2];
        if (n < 0 || want_bytes < 0) return 2;
        uint8_t* comp = (uint8_t*)malloc(n ? (size_t)n : 1);
        uint8_t* want = (uint8_t*)malloc(want_bytes ? (size_t)want_bytes : 1);
        if (!comp || !want || !read_exact(f, comp, (size_t)n) || !read_exact(f, want, (size_t)want_bytes)) return 2;
        // scan
        std::vector<int64_t> cand(1, 0);
        for (int64_t p = 0; p + 4 <= n; ++p)
            if (comp[p] == 0 && comp[p + 1] == 0 && comp[p + 2] == 0xFF && comp[p + 3] == 0xFF) cand.push_back(p + 4);
        const int64_t n_cand = (int64_t)cand.size();
        // segments: every candidate, the speculative ones included
        std::vector<VscReport> rep((size_t)n_cand);
        std::vector<std::vector<uint16_t> > kept((size_t)n_cand);
        for (int64_t c = 0; c < n_cand; ++c) {
            decode(comp, n, cand[c], tables, cells, &rep[c], "record", (long long)rec);
            if (rep[c].status == 0) kept[c].assign(cells.cell, cells.cell + rep[c].produced);
        }
        segments += n_cand;
        // chain
        std::vector<int64_t> chain, offsets;
        int64_t total = 0, at = 0;
        bool ok = true, done = false;
        while (ok && !done) {
            const VscReport& r = rep[at];
            if (r.status != 0 || r.reach > total || total + r.produced > want_bytes) { ok = false; break; }
            chain.push_back(at);
            offsets.push_back(total);
            total += r.produced;
            if (r.final) { done = true; ok = r.end == n; break; }
            int64_t lo = at + 1, hi = n_cand;                          // the candidate whose start is r.end (cand is sorted)
            while (lo < hi) {
                const int64_t mid = (lo + hi) / 2;
                if (cand[mid] < r.end) lo = mid + 1; else hi = mid;
            }
            if (lo >= n_cand || cand[lo] != r.end) { ok = false; break; }
            at = lo;
        }
        if (ok && total != want_bytes) ok = false;
        // place and resolve, into an output with guards
        int64_t produced = 0;
        uint8_t* all = (uint8_t*)malloc((size_t)want_bytes + 2 * GUARD);
        uint8_t* out = all + GUARD;
        memset(all, 0xA5, (size_t)want_bytes + 2 * GUARD);
        if (ok) {
            for (size_t k = 0; k < chain.size(); ++k) {
                const std::vector<uint16_t>& cl = kept[(size_t)chain[k]];
                for (size_t i = 0; i < cl.size(); ++i) out[offsets[k] + (int64_t)i] = (cl[i] & VSC_EXT) ? 0 : (uint8_t)cl[i];
            }
            for (size_t k = 0; k < chain.size(); ++k) {                // chain order: a source is final when it is read
                const std::vector<uint16_t>& cl = kept[(size_t)chain[k]];
                for (size_t i = 0; i < cl.size(); ++i)
                    if (cl[i] & VSC_EXT) out[offsets[k] + (int64_t)i] = out[offsets[k] - 1 - (int64_t)(cl[i] & 0x7fffu)];
            }
            produced = total;
            ++chained;
            if (memcmp(out, want, (size_t)want_bytes) != 0) {
                ++mismatches;
                printf("record %lld: the chain of %zu segments does not give zlib's %lld bytes\n", (long long)rec, chain.size(), (long long)want_bytes);
            }
        }
        for (int i = 0; i < GUARD; ++i)
            if (all[i] != 0xA5 || all[GUARD + want_bytes + i] != 0xA5) {
                ++mismatches;
                printf("record %lld: a guard byte of the output was overwritten\n", (long long)rec);
                break;
            }
        if (mode == 1) {
            VscReport r;
            for (int64_t cut = 0; cut < n; ++cut) {                    // truncated at every byte
                decode(comp, cut, 0, tables, cells, &r, "truncation", (long long)cut);
                if (r.status == 0 && r.end > cut) ++mismatches;
            }
            uint32_t s = 12345u + (uint32_t)rec;
            uint8_t* bad = (uint8_t*)malloc(n ? (size_t)n : 1);
            for (int k = 0; k < 200 && n > 0; ++k) {                   // single-byte corruptions, decoded from every candidate
                s = s * 1664525u + 1013904223u;
                const int64_t where = (int64_t)((s >> 8) % (uint32_t)n);
                s = s * 1664525u + 1013904223u;
                memcpy(bad, comp, (size_t)n);
                bad[where] ^= (uint8_t)(1u + ((s >> 8) % 255u));
                for (int64_t c = 0; c < n_cand; ++c) decode(bad, n, cand[c], tables, cells, &r, "corruption", (long long)k);
            }
            free(bad);
        }
        const int64_t chain_ok = ok ? 1 : 0, chain_len = ok ? (int64_t)chain.size() : 0;
        if (!write_exact(g, &n_cand, 8) || !write_exact(g, &chain_ok, 8) || !write_exact(g, &chain_len, 8) || !write_exact(g, &produced, 8) ||
            !write_exact(g, cand.data(), (size_t)n_cand * 8))
            return 2;
        for (int64_t c = 0; c < n_cand; ++c)
            if (!write_exact(g, &rep[c], sizeof(VscReport))) return 2;
        if (!write_exact(g, chain.data(), (size_t)chain_len * 8) || !write_exact(g, out, (size_t)produced)) return 2;
        free(all);
        free(want);
        free(comp);
    }
    free(tables);
    fclose(f);
    if (fclose(g) != 0) return 2;
    static_assert(sizeof(VscReport) == 8 * VS_INFLATE_REPORT_WORDS, "the report is the words of vs_inflate_segments");
    printf("records %lld chained %ld segments %ld decodes %ld mismatches %ld\n", (long long)records, chained, segments, decodes, mismatches);
    return 0;
}

// Host check of csrc/vs_inflate_blocks_core.h with BOTH finders: what ops.inflate_blocks(stored=True) does on the device, compiled for the
// CPU (with sanitizers where they link) and run on a case file that tests/inflate_stored_inputs.py writes, in the formats of
// tests/host/inflate_blocks_host_check.cpp.  Per record: the candidates are the sorted union of the dynamic finder's (bit 0, and every bit
// where vsb_quick and then vsb_block_start hold) and the stored finder's (every bit where vsb_stored_start holds; the boundary-and-count
// form the kernel uses, vsb_stored_boundary with vsb_stored_count, must give the same positions), then one probe per candidate, the chain
// walk from bit 0, the windows in chain order and the second decode of every span of the chain with its window, compared with the bytes
// zlib produced.  The input, the ring, the tails, the windows and the output are exactly-sized heap buffers (a read or a write outside
// them is a sanitizer report); the output also carries guard bytes on both sides.
//
//   inflate_stored_host_check CASES OUT [LANES]
// LANES (default 1): that many threads play the lanes of the wave; VSI_SYNC, VSC_FENCE and the wave reductions are barriers between them, so
// the striped copies run the way the kernel's do (every lane decodes with the same values, the stores are divided).
// CASES (little-endian): int64 records; per record int64 comp_bytes, int64 out_bytes, int64 mode, the stream, the bytes zlib produced.
// mode 1: the stream is also run through the whole route truncated at each of 64 spread positions and with each of 64 single-bit flips
// (seeded): every such run must end with a failed chain, a CRC-32 other than that of zlib's bytes, or zlib's bytes.
// OUT: int64 records; per record int64 n_cand, chain_ok, chain_len, produced, fail (which chain rule broke, 0 for none), then cand [n_cand],
// words [n_cand * 6], chain (candidate indices) [chain_len], CRC-32 of the windows [chain_len + 1] (as int64), the second decode's words
// [chain_len * 3], the output [produced] (chain_len = produced = 0 unless chain_ok).
// Prints one line per mismatch and a summary line; the exit status is 0 unless a file cannot be read or written.
#include <pthread.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <vector>

static int g_lanes = 1;
static std::atomic<int> g_arrived(0), g_sense(0);
static thread_local int tl_sense = 0, tl_lane = 0;
static int64_t g_reduce[1024];

static void lanes_barrier() {
    if (g_lanes == 1) return;
    tl_sense ^= 1;
    if (g_arrived.fetch_add(1) + 1 == g_lanes) {
        g_arrived.store(0);
        g_sense.store(tl_sense);
    } else {
        while (g_sense.load() != tl_sense) sched_yield();
    }
}
static int64_t lanes_sum(int64_t v) {
    if (g_lanes == 1) return v;
    g_reduce[tl_lane] = v;
    lanes_barrier();
    int64_t s = 0;
    for (int l = 0; l < g_lanes; ++l) s += g_reduce[l];
    lanes_barrier();
    return s;
}
static int lanes_max(int v) {
    if (g_lanes == 1) return v;
    g_reduce[tl_lane] = v;
    lanes_barrier();
    int64_t m = g_reduce[0];
    for (int l = 1; l < g_lanes; ++l) m = g_reduce[l] > m ? g_reduce[l] : m;
    lanes_barrier();
    return (int)m;
}

#define VSI_SYNC() lanes_barrier()
#define VSC_FENCE() lanes_barrier()
#define VSC_WAVE_SUM(v) ((int)lanes_sum(v))
#define VSC_WAVE_MAX(v) lanes_max(v)
#define VSB_WAVE_SUM64(v) lanes_sum(v)
#include "../../spatiotemporal_variable_separation_amd/csrc/vs_inflate_blocks_core.h"

static const int GUARD = 64;

static int read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static int write_exact(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }

static uint32_t g_crc_table[256];
static uint32_t crc32_of(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = g_crc_table[(c ^ p[i]) & 255u] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

// The second decode's sink: the output itself, and the window for what lies before the span.
struct SpanSink {
    uint8_t* out;                              // the span's first output byte
    const uint8_t* window;
    int64_t pos;
    int lane, nlanes;
    uint8_t at(int64_t s) const { return s >= 0 ? out[s] : window[VSB_WINDOW + s]; }
    void lit(uint8_t v) {
        if (lane == 0) out[pos] = v;
        ++pos;
    }
    void copy(int dist, int len) {
        const int64_t sp = pos - dist;
        VSC_FENCE();
        if (dist >= nlanes) {
            for (int j = 0; j < len; j += nlanes) {
                const int i = j + lane;
                if (i < len) out[pos + i] = at(sp + i);
                VSC_FENCE();
            }
        } else {
            for (int j = 0; j < len; j += nlanes) {
                const int i = j + lane;
                if (i < len) out[pos + i] = at(sp + (int)((unsigned)i % (unsigned)dist));
            }
        }
        pos += len;
    }
    void stored(const uint8_t* src, int len) {
        for (int i = lane; i < len; i += nlanes) out[pos + i] = src[i];
        pos += len;
    }
};

// Everything the lanes share about the stream being worked on (written by lane 0 between barriers).
struct Run {
    const uint8_t* comp;
    int64_t n, want_bytes;
    std::vector<int64_t> cand, chain, offsets;
    std::vector<VscReport> rep, rep2;
    std::vector<std::vector<uint16_t> > tails;
    std::vector<std::vector<uint8_t> > windows;
    std::vector<uint8_t> all;                  // GUARD + want_bytes + GUARD
    bool ok;
    int64_t fail;
};
static Run g_run;
static VsiTables* g_tables;
static uint16_t *g_ring, *g_tail;
static long g_mismatches = 0, g_probes = 0, g_spans = 0, g_stored = 0;

// The whole route on g_run.comp[0 .. n); every lane calls it, lane 0 does what one thread does.
static void route(const char* what, long long tag) {
    Run& R = g_run;
    const int lane = tl_lane;
    if (lane == 0) {
        R.cand.assign(1, 0);
        int64_t per_bit = 0;
        for (int64_t bit = 0; bit < R.n * 8; ++bit) {                       // ascending, so the union comes out sorted
            uint64_t w;
            uint32_t hi;
            vsb_peek(R.comp, R.n, bit, &w, &hi);
            const bool dynamic = vsb_quick(w, hi) && vsb_block_start(R.comp, R.n, bit), stored = vsb_stored_start(R.comp, R.n, bit);
            per_bit += stored ? 1 : 0;
            if (bit > 0 && (dynamic || stored)) R.cand.push_back(bit);
        }
        std::vector<int64_t> by_boundary;                                   // the kernel's form: per boundary, how many positions in front of it
        for (int64_t B = 0; B < R.n; ++B) {
            if (!vsb_stored_boundary(R.comp, R.n, B)) continue;
            const uint32_t front = (B >= 2 ? (uint32_t)R.comp[B - 2] : 0xffu) | ((B >= 1 ? (uint32_t)R.comp[B - 1] : 0xffu) << 8);
            for (int k = vsb_stored_count(front) - 1; k >= 0; --k) by_boundary.push_back(8 * B - 3 - k);
        }
        size_t seen = 0;
        for (size_t i = 0; i < by_boundary.size(); ++i)
            if (by_boundary[i] >= 0 && vsb_stored_start(R.comp, R.n, by_boundary[i]) && (i == 0 || by_boundary[i] > by_boundary[i - 1])) ++seen;
        g_stored += per_bit;
        if (seen != by_boundary.size() || (int64_t)seen != per_bit) {
            ++g_mismatches;
            printf("%s %lld: %zu positions by boundary and count, %zu of them stored starts in ascending order, %lld stored starts bit by bit\n", what, tag,
                   by_boundary.size(), seen, (long long)per_bit);
        }
        R.rep.assign(R.cand.size(), VscReport());
        R.tails.assign(R.cand.size(), std::vector<uint16_t>());
    }
    lanes_barrier();
    const int64_t n_cand = (int64_t)R.cand.size();
    for (int64_t c = 0; c < n_cand; ++c) {                               // the probes: every candidate, the false ones included
        if (lane == 0) {
            memset(g_tables, 0xA5, sizeof(VsiTables));
            memset(g_ring, 0x5A, (size_t)VSB_WINDOW * 2);                 // nothing may depend on what a previous probe left
            memset(g_tail, 0x5A, (size_t)VSB_WINDOW * 2);
        }
        lanes_barrier();
        VscReport r;
        vsb_probe(R.comp, R.n, R.cand[c], R.cand.data(), n_cand, g_tables, g_ring, g_tail, &r, lane, g_lanes);
        lanes_barrier();
        if (lane == 0) {
            ++g_probes;
            R.rep[c] = r;
            const int64_t start = R.cand[c];
            const bool sane = r.status >= 0 && r.status <= VS_INFLATE_CAP && r.produced >= 0 && r.end >= start && r.end <= R.n * 8 &&
                              r.end - start <= ((int64_t)VSB_MAX_IN + 1) * 8 && (r.final == 0 || r.final == 1) && r.externals >= 0 &&
                              r.externals <= r.produced && r.reach >= 0 && r.reach <= VSB_WINDOW && (r.externals > 0) == (r.reach > 0) &&
                              (r.final == 0 || r.status == 0) && (r.status != 0 || r.end > start);
            if (!sane) {
                ++g_mismatches;
                printf("%s %lld start %lld: report status %lld end %lld final %lld produced %lld externals %lld reach %lld\n", what, tag, (long long)start,
                       (long long)r.status, (long long)r.end, (long long)r.final, (long long)r.produced, (long long)r.externals, (long long)r.reach);
            }
            if (r.status == 0) R.tails[c].assign(g_tail, g_tail + (r.produced < VSB_WINDOW ? r.produced : VSB_WINDOW));
        }
    }
    if (lane == 0) {                                                        // the chain
        R.chain.clear();
        R.offsets.clear();
        R.ok = true;
        R.fail = 0;
        int64_t total = 0, at = 0;
        for (;;) {
            const VscReport& r = R.rep[at];
            if (r.status != 0) { R.ok = false; R.fail = 1; break; }
            if (r.reach > total) { R.ok = false; R.fail = 2; break; }
            if (total + r.produced > R.want_bytes) { R.ok = false; R.fail = 3; break; }
            R.chain.push_back(at);
            R.offsets.push_back(total);
            total += r.produced;
            if (r.final) {
                if ((r.end + 7) / 8 != R.n) { R.ok = false; R.fail = 4; }
                break;
            }
            int64_t lo = at + 1, hi = n_cand;
            while (lo < hi) {
                const int64_t mid = (lo + hi) / 2;
                if (R.cand[mid] < r.end) lo = mid + 1; else hi = mid;
            }
            if (lo >= n_cand || R.cand[lo] != r.end) { R.ok = false; R.fail = 5; break; }
            at = lo;
        }
        if (R.ok && total != R.want_bytes) { R.ok = false; R.fail = 6; }
        R.all.assign((size_t)R.want_bytes + 2 * GUARD, 0xA5);
        R.windows.clear();
        R.rep2.clear();
        if (R.ok) {                                                         // the windows, in chain order
            R.windows.assign(R.chain.size() + 1, std::vector<uint8_t>());
            R.windows[0].assign(VSB_WINDOW, 0);
            for (size_t k = 0; k < R.chain.size(); ++k) {
                const std::vector<uint16_t>& tail = R.tails[(size_t)R.chain[k]];
                R.windows[k + 1].resize(VSB_WINDOW);
                for (int j = 0; j < VSB_WINDOW; ++j)
                    R.windows[k + 1][j] = vsb_window_byte(R.windows[k].data(), tail.data(), R.rep[(size_t)R.chain[k]].produced, j);
            }
            R.rep2.assign(R.chain.size(), VscReport());
        }
    }
    lanes_barrier();
    if (!R.ok) return;
    for (size_t k = 0; k < R.chain.size(); ++k) {                           // the second decode, straight into the output
        const VscReport& first = R.rep[(size_t)R.chain[k]];
        if (lane == 0) memset(g_tables, 0xA5, sizeof(VsiTables));
        lanes_barrier();
        SpanSink sink;
        sink.out = R.all.data() + GUARD + R.offsets[k];
        sink.window = R.windows[k].data();
        sink.pos = 0; sink.lane = lane; sink.nlanes = g_lanes;
        VscReport r;
        vsb_inflate_span(R.comp, R.n, R.cand[(size_t)R.chain[k]], (const int64_t*)nullptr, (int64_t)0, first.end, first.produced,
                         R.offsets[k] < VSB_WINDOW ? R.offsets[k] : (int64_t)VSB_WINDOW, g_tables, sink, &r);
        lanes_barrier();
        if (lane == 0) {
            ++g_spans;
            R.rep2[k] = r;
            if (r.status != first.status || r.end != first.end || r.produced != first.produced) {
                ++g_mismatches;
                printf("%s %lld span %zu: the second decode reports status %lld end %lld produced %lld, the probe %lld %lld %lld\n", what, tag, k,
                       (long long)r.status, (long long)r.end, (long long)r.produced, (long long)first.status, (long long)first.end, (long long)first.produced);
            }
        }
    }
    lanes_barrier();
    if (lane == 0)
        for (int i = 0; i < GUARD; ++i)
            if (R.all[i] != 0xA5 || R.all[GUARD + R.want_bytes + i] != 0xA5) {
                ++g_mismatches;
                printf("%s %lld: a guard byte of the output was overwritten\n", what, tag);
                break;
            }
}

static FILE *g_in, *g_out;
static int g_io_error = 0;
static long g_chained = 0, g_damaged = 0, g_damaged_right = 0, g_damaged_chained = 0;

static void* lane_main(void* arg) {
    tl_lane = (int)(intptr_t)arg;
    const int lane = tl_lane;
    static int64_t records = 0;
    if (lane == 0 && (!read_exact(g_in, &records, 8) || !write_exact(g_out, &records, 8))) { g_io_error = 1; records = 0; }
    lanes_barrier();
    for (int64_t rec = 0; rec < records; ++rec) {
        static uint8_t *comp, *want, *bad;
        static int64_t n, want_bytes, mode;
        if (lane == 0) {
            int64_t head[3] = {0, 0, 0};
            if (!read_exact(g_in, head, sizeof(head)) || head[0] < 0 || head[1] < 0) { g_io_error = 1; head[0] = head[1] = head[2] = 0; }
            n = head[0]; want_bytes = head[1]; mode = head[2];
            comp = (uint8_t*)malloc(n ? (size_t)n : 1);
            want = (uint8_t*)malloc(want_bytes ? (size_t)want_bytes : 1);
            if (!read_exact(g_in, comp, (size_t)n) || !read_exact(g_in, want, (size_t)want_bytes)) g_io_error = 1;
            g_run.comp = comp; g_run.n = n; g_run.want_bytes = want_bytes;
        }
        lanes_barrier();
        route("record", (long long)rec);
        if (lane == 0) {
            Run& R = g_run;
            const uint8_t* out = R.all.data() + GUARD;
            if (R.ok) {
                ++g_chained;
                if (memcmp(out, want, (size_t)want_bytes) != 0) {
                    ++g_mismatches;
                    printf("record %lld: the chain of %zu spans does not give zlib's %lld bytes\n", (long long)rec, R.chain.size(), (long long)want_bytes);
                }
            }
            const int64_t n_cand = (int64_t)R.cand.size(), chain_ok = R.ok ? 1 : 0, chain_len = R.ok ? (int64_t)R.chain.size() : 0,
                          produced = R.ok ? want_bytes : 0;
            int fine = write_exact(g_out, &n_cand, 8) && write_exact(g_out, &chain_ok, 8) && write_exact(g_out, &chain_len, 8) &&
                       write_exact(g_out, &produced, 8) && write_exact(g_out, &R.fail, 8) && write_exact(g_out, R.cand.data(), (size_t)n_cand * 8);
            for (int64_t c = 0; c < n_cand && fine; ++c) fine = write_exact(g_out, &R.rep[(size_t)c], sizeof(VscReport));
            if (R.ok) {
                fine = fine && write_exact(g_out, R.chain.data(), (size_t)chain_len * 8);
                for (int64_t k = 0; k <= chain_len && fine; ++k) {
                    const int64_t crc = crc32_of(R.windows[(size_t)k].data(), VSB_WINDOW);
                    fine = write_exact(g_out, &crc, 8);
                }
                for (int64_t k = 0; k < chain_len && fine; ++k) {
                    const int64_t w[3] = {R.rep2[(size_t)k].status, R.rep2[(size_t)k].end, R.rep2[(size_t)k].produced};
                    fine = write_exact(g_out, w, sizeof(w));
                }
                fine = fine && write_exact(g_out, out, (size_t)produced);
            } else {
                const int64_t crc = 0;                                      // chain_len = 0: the one window before the stream
                fine = fine && write_exact(g_out, &crc, 8);
            }
            if (!fine) g_io_error = 1;
            bad = (uint8_t*)malloc(n ? (size_t)n : 1);
        }
        lanes_barrier();
        if (mode == 1) {
            const uint32_t want_crc = crc32_of(want, (size_t)want_bytes);
            uint32_t s = 12345u + (uint32_t)rec;
            for (int k = 0; k < 128 && n > 0; ++k) {                        // 64 truncations at spread positions, then 64 single-bit flips
                if (lane == 0) {
                    memcpy(bad, comp, (size_t)n);
                    g_run.comp = bad;
                    if (k < 64) {
                        g_run.n = n * (k + 1) / 65;
                    } else {
                        s = s * 1664525u + 1013904223u;
                        const int64_t where = (int64_t)((s >> 4) % (uint32_t)(n * 8 > 0x7fffffff ? 0x7fffffff : n * 8));
                        bad[where >> 3] ^= (uint8_t)(1u << (where & 7));
                        g_run.n = n;
                    }
                    // an exactly-sized copy, so that a read behind a truncation is a sanitizer report
                    uint8_t* exact = (uint8_t*)malloc(g_run.n ? (size_t)g_run.n : 1);
                    memcpy(exact, bad, (size_t)g_run.n);
                    g_run.comp = exact;
                }
                lanes_barrier();
                route(k < 64 ? "truncation" : "flip", (long long)k);
                if (lane == 0) {
                    ++g_damaged;
                    const uint8_t* out = g_run.all.data() + GUARD;
                    if (g_run.ok) ++g_damaged_chained;                      // (a flip inside a stored block's bytes: only the CRC-32 can tell)
                    if (g_run.ok && crc32_of(out, (size_t)want_bytes) == want_crc) {
                        ++g_damaged_right;
                        if (memcmp(out, want, (size_t)want_bytes) != 0) {
                            ++g_mismatches;
                            printf("record %lld damage %d: wrong bytes under a right CRC-32\n", (long long)rec, k);
                        }
                    }
                    free((void*)g_run.comp);
                }
                lanes_barrier();
            }
        }
        if (lane == 0) {
            free(bad);
            free(want);
            free(comp);
        }
        lanes_barrier();
    }
    return nullptr;
}

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) return 2;
    g_lanes = argc == 4 ? atoi(argv[3]) : 1;
    if (g_lanes < 1 || g_lanes > 1024) return 2;
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) return 2;
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        g_crc_table[i] = c;
    }
    g_tables = (VsiTables*)malloc(sizeof(VsiTables));
    g_ring = (uint16_t*)malloc((size_t)VSB_WINDOW * 2);
    g_tail = (uint16_t*)malloc((size_t)VSB_WINDOW * 2);
    std::vector<pthread_t> threads((size_t)g_lanes);
    for (int l = 1; l < g_lanes; ++l)
        if (pthread_create(&threads[(size_t)l], nullptr, lane_main, (void*)(intptr_t)l) != 0) return 3;
    lane_main((void*)(intptr_t)0);
    for (int l = 1; l < g_lanes; ++l) pthread_join(threads[(size_t)l], nullptr);
    free(g_tail);
    free(g_ring);
    free(g_tables);
    fclose(g_in);
    if (fclose(g_out) != 0 || g_io_error) return 2;
    static_assert(sizeof(VscReport) == 8 * VS_INFLATE_REPORT_WORDS, "the report is the words of vs_inflate_block_probe");
    printf("lanes %d chained %ld stored_starts %ld probes %ld spans %ld damaged %ld damaged_right %ld damaged_chained %ld mismatches %ld\n", g_lanes,
           g_chained, g_stored, g_probes, g_spans, g_damaged, g_damaged_right, g_damaged_chained, g_mismatches);
    return 0;
}

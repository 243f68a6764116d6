// Host check of csrc/vs_mt19937_core.h: the logic of vs_mt19937_randint, compiled for the CPU (with sanitizers where they link) and run on
// a file of cases that tests/test_mmnist_draws_cpu.py writes.  Every call fills an exactly-sized heap table from an exactly-sized heap
// copy of the state, so that a read or a write outside either is a sanitizer report.  The tables and the final states go to an output
// file, where the test compares them with NumPy's and the GPU test with the kernel's.
//
// Two builds of this file.  Plain: the header's own one-lane defaults of the lane primitives.  With -DVSM_HOST_LANES: LANES threads play
// the lanes of a workgroup -- a barrier for VSM_SYNC, the scans through a shared array -- so that the windowed, scanned form the kernel
// runs is the form checked here, at a lane count of the caller's choice.
//
//   mt19937_host_check CASES OUT LANES          (LANES must be 1 for the plain build, 1 .. 1024 for the other)
// CASES (little-endian): int64 cases; per case uint32 state[625], int32 k, int32 lows[8], int32 highs[8], int32 calls, int64 rows[calls].
// OUT: int64 cases; per case and call int32 status and, when the status is 0, int32 table[rows * k]; per case uint32 state[625] at its end.
// The exit status is 0 unless a file cannot be read or written or the arguments are wrong.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#ifdef VSM_HOST_LANES
#include <pthread.h>
#include <stdint.h>
static pthread_barrier_t g_barrier;
static uint32_t g_maps[1024];
static int g_adds[1024];
static thread_local int t_lane;
static int g_lanes;
static void host_scan_map(uint32_t m, uint32_t& before, uint32_t& total);
static void host_scan_add(int v, int& before, int& total);
#define VSM_SYNC() ((void)pthread_barrier_wait(&g_barrier))
#define VSM_SCAN_MAP(m, before, total) host_scan_map((m), (before), (total))
#define VSM_SCAN_ADD(v, before, total) host_scan_add((v), (before), (total))
#endif

#include "../../spatiotemporal_variable_separation_amd/csrc/vs_mt19937_core.h"

#ifdef VSM_HOST_LANES
static void host_scan_map(uint32_t m, uint32_t& before, uint32_t& total) {
    g_maps[t_lane] = m;
    pthread_barrier_wait(&g_barrier);
    uint32_t acc = VSM_IDENTITY;
    for (int i = 0; i < g_lanes; ++i) {
        if (i == t_lane) before = acc;
        acc = vsm_compose(acc, g_maps[i]);
    }
    total = acc;
    pthread_barrier_wait(&g_barrier);               // the array is free for the next scan
}
static void host_scan_add(int v, int& before, int& total) {
    g_adds[t_lane] = v;
    pthread_barrier_wait(&g_barrier);
    int acc = 0;
    for (int i = 0; i < g_lanes; ++i) {
        if (i == t_lane) before = acc;
        acc += g_adds[i];
    }
    total = acc;
    pthread_barrier_wait(&g_barrier);
}

struct LaneCall {
    uint32_t* state;
    VsmWork* work;
    const VsmCols* cols;
    int64_t rows;
    int32_t* out;
    int lane, status;
};
static void* lane_main(void* p) {
    LaneCall* c = (LaneCall*)p;
    t_lane = c->lane;
    c->status = vsm_fill_table(c->state, c->work, c->cols, c->rows, c->out, c->lane, g_lanes);
    return nullptr;
}
#endif

static int fill(uint32_t* state, VsmWork* work, const VsmCols* cols, int64_t rows, int32_t* out, int lanes) {
#ifdef VSM_HOST_LANES
    std::vector<LaneCall> calls((size_t)lanes);
    std::vector<pthread_t> threads((size_t)lanes);
    for (int l = 0; l < lanes; ++l) {
        calls[l] = LaneCall{state, work, cols, rows, out, l, -1};
        if (pthread_create(&threads[l], nullptr, lane_main, &calls[l]) != 0) exit(3);
    }
    for (int l = 0; l < lanes; ++l) pthread_join(threads[l], nullptr);
    for (int l = 1; l < lanes; ++l)
        if (calls[l].status != calls[0].status) return -100;          // the status is uniform over the lanes
    return calls[0].status;
#else
    (void)lanes;
    return vsm_fill_table(state, work, cols, rows, out, 0, 1);
#endif
}

static int read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static int write_exact(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int lanes = atoi(argv[3]);
#ifdef VSM_HOST_LANES
    if (lanes < 1 || lanes > 1024) return 2;
    g_lanes = lanes;
    if (pthread_barrier_init(&g_barrier, nullptr, (unsigned)lanes) != 0) return 3;
#else
    if (lanes != 1) return 2;
#endif
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    if (!f || !g) return 1;
    int64_t cases = 0;
    if (!read_exact(f, &cases, 8) || !write_exact(g, &cases, 8)) return 1;
    int64_t calls_made = 0;
    for (int64_t c = 0; c < cases; ++c) {
        uint32_t* state = (uint32_t*)malloc(VSM_STATE_WORDS * sizeof(uint32_t));   // exactly the state: nothing outside it may be touched
        int32_t k, lows[VSM_MAX_COLS], highs[VSM_MAX_COLS], n_calls;
        if (!read_exact(f, state, VSM_STATE_WORDS * 4) || !read_exact(f, &k, 4) || !read_exact(f, lows, sizeof lows) ||
            !read_exact(f, highs, sizeof highs) || !read_exact(f, &n_calls, 4))
            return 1;
        if (k < 1 || k > VSM_MAX_COLS || n_calls < 0) return 2;
        VsmCols cols;
        vsm_cols_init(&cols, lows, highs, k);
        VsmWork* work = (VsmWork*)malloc(sizeof(VsmWork));
        for (int32_t call = 0; call < n_calls; ++call) {
            int64_t rows;
            if (!read_exact(f, &rows, 8) || rows < 0) return 1;
            const size_t n = (size_t)rows * (size_t)k;
            int32_t* out = (int32_t*)malloc(n ? n * sizeof(int32_t) : 1);
            const int32_t status = rows == 0 ? VSM_STATUS_OK : fill(state, work, &cols, rows, out, lanes);   // the entry point launches nothing for 0 rows
            if (!write_exact(g, &status, 4)) return 1;
            if (status == VSM_STATUS_OK && !write_exact(g, out, n * sizeof(int32_t))) return 1;
            free(out);
            ++calls_made;
        }
        if (!write_exact(g, state, VSM_STATE_WORDS * 4)) return 1;
        free(work);
        free(state);
    }
    if (fclose(g) != 0) return 1;
    fclose(f);
    printf("cases %lld calls %lld lanes %d\n", (long long)cases, (long long)calls_made, lanes);
    return 0;
}

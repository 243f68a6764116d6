// Host check of csrc/vs_mmnist_walk_core.h: the logic of vs_mmnist_stochastic_trajectories, compiled for the CPU (with sanitizers where they
// link) and run on a file of cases that tests/smnist_inputs.py writes.  Every call fills exactly-sized heap tables from an exactly-sized
// heap copy of the state, so that a read or a write outside any of them is a sanitizer report.  The tables and the final states go to an
// output file, where the tests compare them with the fixture, with the NumPy-driven restatement and with the kernel's.
//
// Two builds of this file.  Plain: the core's one-lane form (vsw_walk_serial).  With -DVSW_HOST_LANES: the lanes form (vsw_walk_lanes),
// LANES threads playing the lanes of a workgroup with a barrier for VSM_SYNC -- the speculative form the kernel runs, at a lane count of
// the caller's choice.
//
//   mmnist_walk_host_check CASES OUT LANES      (LANES must be 1 for the plain build, 1 .. 1024 for the other)
// CASES (little-endian): int64 cases; per case uint32 state[625], int32 n_pre, seq_len, x_max, y_max, max_speed, want_latents, desc_nd (0:
// no desc), calls, int32 lows[5], int32 highs[5]; per call int64 n_traj and, when n_pre < 4, int32 start[n_traj * 4].
// OUT: int64 cases; per case and call int32 status and, when the status is 0, int32 pre[n_traj * n_pre], positions[seq_len * n_traj * 2],
// latents[seq_len * n_traj * 4] (if wanted), desc[n_traj / nd * (1 + nd)] (if wanted); per case uint32 state[625] at its end.
// The exit status is 0 unless a file cannot be read or written or the arguments are wrong.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#ifdef VSW_HOST_LANES
#include <pthread.h>
static pthread_barrier_t g_barrier;
#define VSM_SYNC() ((void)pthread_barrier_wait(&g_barrier))
#define VSM_SCAN_MAP(m, before, total) ((before) = VSM_IDENTITY, (total) = (m))      /* vsm_fill_table's: not called here */
#define VSM_SCAN_ADD(v, before, total) ((before) = 0, (total) = (v))
#endif

#include "../../spatiotemporal_variable_separation_amd/csrc/vs_mmnist_walk_core.h"

struct Call {
    uint32_t* state;
    VswWork* work;
    const VswGeom* geom;
    int64_t n_traj;
    const int32_t* start;
    int32_t *pre, *positions, *latents, *desc;
    int nd, lane, lanes, status;
};

#ifdef VSW_HOST_LANES
static void* lane_main(void* p) {
    Call* c = (Call*)p;
    c->status = vsw_walk_lanes(c->state, c->work, c->geom, c->n_traj, c->start, c->pre, c->positions, c->latents, c->desc, c->nd, c->lane, c->lanes);
    return nullptr;
}
#endif

static int walk(Call call) {
#ifdef VSW_HOST_LANES
    std::vector<Call> calls((size_t)call.lanes, call);
    std::vector<pthread_t> threads((size_t)call.lanes);
    for (int l = 0; l < call.lanes; ++l) {
        calls[l].lane = l;
        if (pthread_create(&threads[l], nullptr, lane_main, &calls[l]) != 0) exit(3);
    }
    for (int l = 0; l < call.lanes; ++l) pthread_join(threads[l], nullptr);
    for (int l = 1; l < call.lanes; ++l)
        if (calls[l].status != calls[0].status) return -100;          // the status is uniform over the lanes
    return calls[0].status;
#else
    return vsw_walk_serial(call.state, call.work, call.geom, call.n_traj, call.start, call.pre, call.positions, call.latents, call.desc, call.nd);
#endif
}

static int read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static int write_exact(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }
static int32_t* table(size_t n) { return (int32_t*)malloc(n ? n * sizeof(int32_t) : 1); }

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int lanes = atoi(argv[3]);
#ifdef VSW_HOST_LANES
    if (lanes < 1 || lanes > 1024) return 2;
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
        int32_t head[8], lows[5], highs[5];
        if (!read_exact(f, state, VSM_STATE_WORDS * 4) || !read_exact(f, head, sizeof head) || !read_exact(f, lows, sizeof lows) ||
            !read_exact(f, highs, sizeof highs))
            return 1;
        const int n_pre = head[0], seq_len = head[1], x_max = head[2], y_max = head[3], max_speed = head[4], want_latents = head[5], nd = head[6];
        const int n_calls = head[7];
        if (n_pre < 0 || n_pre > 5 || seq_len < 1 || x_max < 1 || y_max < 1 || max_speed < 0 || nd < 0 || n_calls < 0) return 2;
        VswGeom geom;
        vsw_geom_init(&geom, n_pre, seq_len, lows, highs, x_max, y_max, max_speed);
        VswWork* work = (VswWork*)malloc(sizeof(VswWork));
        for (int32_t call = 0; call < n_calls; ++call) {
            int64_t n;
            if (!read_exact(f, &n, 8) || n < 0 || (nd && n % nd)) return 1;
            const size_t sn = (size_t)n, st = (size_t)seq_len;
            int32_t* start = n_pre < 4 ? table(sn * 4) : nullptr;
            if (start && !read_exact(f, start, sn * 16)) return 1;
            int32_t* pre = n_pre ? table(sn * (size_t)n_pre) : nullptr;
            int32_t* positions = table(st * sn * 2);
            int32_t* latents = want_latents ? table(st * sn * 4) : nullptr;
            int32_t* desc = nd ? table(sn / (size_t)nd * (size_t)(1 + nd)) : nullptr;
            // the entry point launches nothing for 0 trajectories
            const int32_t status = n == 0 ? VSM_STATUS_OK : walk(Call{state, work, &geom, n, start, pre, positions, latents, desc, nd ? nd : 1, 0, lanes, -1});
            if (!write_exact(g, &status, 4)) return 1;
            if (status == VSM_STATUS_OK) {
                if (!write_exact(g, pre, sn * (size_t)n_pre * 4) || !write_exact(g, positions, st * sn * 8)) return 1;
                if (latents && !write_exact(g, latents, st * sn * 16)) return 1;
                if (desc && !write_exact(g, desc, sn / (size_t)nd * (size_t)(1 + nd) * 4)) return 1;
            }
            free(start); free(pre); free(positions); free(latents); free(desc);
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

// Host check of csrc/vs_mmnist_bounce_core.h: the deterministic Moving-MNIST walker that csrc/vs_data.hip runs, compiled for the CPU (with
// sanitizers where they link) and run on a file of start states that tests/test_mmnist_bounce_cpu.py writes.  Every trajectory fills an
// exactly-sized heap table, so that a write outside it is a sanitizer report.  The rows go to an output file, where the test compares
// them with oracle/mmnist_ref.py.
//
//   mmnist_bounce_host_check CASES OUT
// CASES (little-endian): int64 groups; per group int32 x_max, y_max, seq_len, t0, n and int32 start[n][4] = (row, column, row speed, column
// speed).  Frames before t0 are walked and not recorded.
// OUT: int64 groups; per group and trajectory int32 frames that gave up on the pass budget, then int32 rows[seq_len - t0][4] = (row,
// column, row speed, column speed).
// The exit status is 0 unless a file cannot be read or written or the arguments are wrong.
#include <stdio.h>
#include <stdlib.h>

#include "../../spatiotemporal_variable_separation_amd/csrc/vs_mmnist_bounce_core.h"

static int read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static int write_exact(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    if (!f || !g) return 1;
    int64_t groups = 0, walked = 0, gave_up_total = 0;
    if (!read_exact(f, &groups, 8) || !write_exact(g, &groups, 8)) return 1;
    for (int64_t k = 0; k < groups; ++k) {
        int32_t head[5];
        if (!read_exact(f, head, sizeof head)) return 1;
        const int x_max = head[0], y_max = head[1], seq_len = head[2], t0 = head[3], n = head[4];
        if (x_max < 0 || y_max < 0 || seq_len < 1 || t0 < 0 || t0 >= seq_len || n < 0) return 2;
        const size_t rows = (size_t)(seq_len - t0);
        for (int i = 0; i < n; ++i) {
            int32_t q[4];
            if (!read_exact(f, q, sizeof q)) return 1;
            int32_t* out = (int32_t*)malloc(rows * 4 * sizeof(int32_t));    // exactly the rows: nothing outside them may be touched
            const int32_t gave_up = vsw_walk_deterministic(x_max, y_max, q[0], q[1], q[2], q[3], t0, seq_len, [&](int t, const int32_t* row) {
                for (int c = 0; c < 4; ++c) out[(size_t)(t - t0) * 4 + c] = row[c];
            });
            if (!write_exact(g, &gave_up, 4) || !write_exact(g, out, rows * 4 * sizeof(int32_t))) return 1;
            free(out);
            ++walked;
            gave_up_total += gave_up;
        }
    }
    if (fclose(g) != 0) return 1;
    fclose(f);
    printf("groups %lld trajectories %lld frames_on_the_pass_budget %lld\n", (long long)groups, (long long)walked, (long long)gave_up_total);
    return 0;
}

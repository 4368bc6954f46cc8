// tsdf_sample_plan_run.cpp -- csrc/tsdfsample_plan.h run on the host: the sample of a fused state at posed queries and the sum of the
// Gauss-Newton records of one registration step, by the very functions the kernels of csrc/tsdficp.hip loop around.  A stand-alone
// program for tests/test_tsdf_sample_cpu.py, built plain and under AddressSanitizer / UBSan.
//   stdin   "constants", or: nx ny nz min_obs has_g b, origin[3] voxel trunc (hex float64), g[12] (hex fp32, with has_g), then nx ny nz
//           ints of sum, as many of n, then b rows of three hex fp32
//   stdout  b lines "state phi grad0 grad1 grad2" (hex float64), one line of the three counts, one line of the 28 summed moments
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tsdfsample_plan.h"

using namespace ls::ts;

// the posed query: the expression of ls_cloud_merge_f32 as csrc/cloud_grid.h states it (pose_row), every product and sum rounded to fp32
static void pose_row(const float* g, float x0, float x1, float x2, float (&y)[3]) {
    y[0] = x0, y[1] = x1, y[2] = x2;
    if (g)
        for (int r = 0; r < 3; ++r) y[r] = ((g[r * 4 + 0] * x0 + g[r * 4 + 1] * x1) + g[r * 4 + 2] * x2) + g[r * 4 + 3];
}

static bool read_token(char* buf, size_t n) { return scanf("%63s", buf) == 1 && n >= 64; }

int main() {
    char tok[64];
    if (!read_token(tok, sizeof tok)) return 2;
    if (tok[0] == 'c') {
        printf("%d %d %d %d %d %d\n", SAMPLE_CHUNK, SAMPLE_WAVE, SAMPLE_GRID_WORDS, GN_MOMENTS, SAMPLE_STATES, CNT_FIELDS);
        return 0;
    }
    int dims[3], min_obs, has_g;
    long long b;
    dims[0] = atoi(tok);
    if (scanf("%d %d %d %d %lld", &dims[1], &dims[2], &min_obs, &has_g, &b) != 5 || dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || b < 0) return 2;
    double grid[5];
    for (double& v : grid) {
        if (!read_token(tok, sizeof tok)) return 2;
        v = strtod(tok, nullptr);
    }
    float g[12];
    if (has_g)
        for (float& v : g) {
            if (!read_token(tok, sizeof tok)) return 2;
            v = strtof(tok, nullptr);
        }
    const size_t voxels = (size_t)dims[0] * dims[1] * dims[2];
    std::vector<int> S(voxels), N(voxels);
    for (int& v : S)
        if (scanf("%d", &v) != 1) return 2;
    for (int& v : N)
        if (scanf("%d", &v) != 1) return 2;
    const double trunc = grid[4], toh = sample_trunc_over_h(grid[3], trunc);
    std::vector<double> mom((size_t)b * GN_MOMENTS);
    long long counts[CNT_FIELDS] = {0, 0, 0};
    for (long long q = 0; q < b; ++q) {
        float x[3], y[3];
        for (float& v : x) {
            if (!read_token(tok, sizeof tok)) return 2;
            v = strtof(tok, nullptr);
        }
        pose_row(has_g ? g : nullptr, x[0], x[1], x[2], y);
        int i[3], what = SAMPLE_OUT;
        double f[3], phi = trunc, grad[3] = {0.0, 0.0, 0.0};
        bool finite;
        if (sample_cell(y, grid, grid[3], dims, i, f, &finite)) {
            int s[8], n[8];
            for (int c = 0; c < 8; ++c) {
                const long long at = sample_corner(dims, i, c);
                s[c] = S.at((size_t)at);
                n[c] = N.at((size_t)at);
            }
            what = sample_value(s, n, min_obs, f, trunc, toh, &phi, grad);
        }
        counts[CNT_FINITE] += finite, counts[CNT_INSIDE] += what != SAMPLE_OUT, counts[CNT_SAMPLED] += what == SAMPLE_SAMPLED;
        double m[GN_MOMENTS];
        gn_record(what == SAMPLE_SAMPLED, phi, y, grad, m);
        for (int e = 0; e < GN_MOMENTS; ++e) mom[(size_t)q * GN_MOMENTS + e] = m[e];
        printf("%d %a %a %a %a\n", what, phi, grad[0], grad[1], grad[2]);
    }
    printf("%lld %lld %lld\n", counts[0], counts[1], counts[2]);
    for (int e = 0; e < GN_MOMENTS; ++e) {
        double s = 0.0;
        for (long long c = 0; c < sample_chunks(b); ++c) {
            const long long left = b - c * SAMPLE_CHUNK;
            s += sample_chunk_record(mom.data() + (size_t)c * SAMPLE_CHUNK * GN_MOMENTS + e, (int)(left < SAMPLE_CHUNK ? left : SAMPLE_CHUNK), GN_MOMENTS);
        }
        printf("%a%c", s, e + 1 < GN_MOMENTS ? ' ' : '\n');
    }
    return 0;
}

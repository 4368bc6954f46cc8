// tsdfprior_plan_run.cpp -- csrc/tsdfprior_plan.h run on the host: the query rows of the samples the prior votes at and the completed
// state, by the very functions the kernels of csrc/tsdfprior.hip loop around.  A stand-alone program for tests/test_tsdf_prior_cpu.py,
// built plain and under AddressSanitizer / UBSan.
//   stdin   "constants", or
//           "checks" w0 s (hex float64) P nx ny nz, or
//           "complete" nx ny nz w0 R, origin[3] voxel trunc s (hex float64), then nx ny nz ints of sum and as many of n, then R values
//           (hex fp32 or nan / inf / -inf) in row order
//   stdout  checks: "bad_weight bad_scale bad_sizes sizes_ok"
//           complete: R lines "index p0 p1 p2" (hex), one line of sum', one of n', one of the four counts
//   exit    4: R is not the number of eligible samples
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tsdfprior_plan.h"

using namespace ls::tp;

static bool read_token(char* buf, size_t n) { return scanf("%63s", buf) == 1 && n >= 64; }
static bool read_double(double* v) {
    char tok[64];
    if (!read_token(tok, sizeof tok)) return false;
    *v = strtod(tok, nullptr);
    return true;
}
static bool read_float(float* v) {
    char tok[64];
    if (!read_token(tok, sizeof tok)) return false;
    *v = strtof(tok, nullptr);
    return true;
}

static int run_checks() {
    int w0, P, nx, ny, nz;
    double s;
    if (scanf("%d", &w0) != 1 || !read_double(&s) || scanf("%d %d %d %d", &P, &nx, &ny, &nz) != 4) return 2;
    const bool ok = ls::fp::fuse_sizes_ok(P, nx, ny, nz);
    printf("%d %d %d %d\n", prior_bad_weight(w0), prior_bad_scale(s), ok ? prior_bad_sizes(P, nx, ny, nz) : -1, (int)ok);
    return 0;
}

static int run_complete() {
    int dims[3], w0;
    long long R;
    if (scanf("%d %d %d %d %lld", &dims[0], &dims[1], &dims[2], &w0, &R) != 5) return 2;
    if (!ls::fp::fuse_sizes_ok(1, dims[0], dims[1], dims[2]) || prior_bad_sizes(1, dims[0], dims[1], dims[2]) != 0 || prior_bad_weight(w0) != 0 || R < 0)
        return 3;
    double grid[PRIOR_GRID_WORDS];
    for (double& v : grid)
        if (!read_double(&v)) return 2;
    if (ls::fp::fuse_bad_grid(grid, grid[3], grid[4]) != 0 || prior_bad_scale(grid[5]) != 0) return 3;
    const size_t voxels = (size_t)dims[0] * dims[1] * dims[2];
    std::vector<int> S(voxels), N(voxels), So(voxels), No(voxels);
    for (int& v : S)
        if (scanf("%d", &v) != 1) return 2;
    for (int& v : N)
        if (scanf("%d", &v) != 1) return 2;
    std::vector<float> f((size_t)R);
    for (float& v : f)
        if (!read_float(&v)) return 2;
    long long counts[PRIOR_FIELDS] = {0, 0, 0, 0}, row = 0;
    for (size_t i = 0; i < voxels; ++i) {
        const bool eligible = prior_weight(w0, N[i]) > 0;
        if (eligible && row >= R) return 4;
        const int did = prior_vote(S[i], N[i], w0, grid[5], grid[4], eligible ? f.at((size_t)row) : 0.0f, &So[i], &No[i]);
        if (eligible) {
            float point[3];
            prior_row((long long)i, dims, grid, grid[3], point);
            printf("%zu %a %a %a\n", i, (double)point[0], (double)point[1], (double)point[2]);
            ++row;
        }
        counts[PRIOR_ELIGIBLE] += eligible;
        counts[did == VOTE_CAST ? PRIOR_VOTED : (did == VOTE_SKIPPED ? PRIOR_SKIPPED : PRIOR_UNTOUCHED)] += 1;
    }
    if (row != R) return 4;
    for (size_t i = 0; i < voxels; ++i) printf("%d%c", So[i], i + 1 < voxels ? ' ' : '\n');
    for (size_t i = 0; i < voxels; ++i) printf("%d%c", No[i], i + 1 < voxels ? ' ' : '\n');
    printf("%lld %lld %lld %lld\n", counts[0], counts[1], counts[2], counts[3]);
    return 0;
}

int main() {
    char tok[64];
    if (!read_token(tok, sizeof tok)) return 2;
    if (!strcmp(tok, "constants")) {
        printf("%d %d %d %d %d %d %d %d %d %d %d\n", PRIOR_ELIGIBLE, PRIOR_VOTED, PRIOR_SKIPPED, PRIOR_UNTOUCHED, PRIOR_FIELDS, PRIOR_WORD, PRIOR_BLOCK_WORDS,
               PRIOR_BLOCK, PRIOR_MAX_BLOCKS, PRIOR_MAX_WEIGHT, PRIOR_GRID_WORDS);
        return 0;
    }
    if (!strcmp(tok, "checks")) return run_checks();
    if (!strcmp(tok, "complete")) return run_complete();
    return 2;
}

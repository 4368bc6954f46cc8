// tsdffit_plan_run.cpp -- csrc/tsdffit_plan.h run on the host: the draw of band and free-space samples out of a fused state and the fit
// loss, by the very functions the kernels of csrc/tsdffit.hip loop around.  A stand-alone program for tests/test_tsdf_fit_cpu.py, built
// plain and under AddressSanitizer / UBSan.
//   stdin   "constants", or
//           "draw" nx ny nz min_obs n_band n_free seed (decimal uint64), origin[3] voxel trunc (hex float64), then nx ny nz ints of sum
//           and as many of n, or
//           "loss" P N has_min, then per problem: s (hex fp32) trunc (hex float64) [min_loss (hex float64)] and N triples
//           "kind sdf target" (int, hex fp32, hex float64)
//   stdout  draw: N lines "kind index target p0 p1 p2" (hex), one line of the three counts
//           loss: per problem one line "loss min_loss improved" and one line of the N gradients (hex)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tsdffit_plan.h"

using namespace ls::tf;

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

static int run_draw() {
    int dims[3], min_obs;
    long long n_band, n_free;
    unsigned long long seed;
    if (scanf("%d %d %d %d %lld %lld %llu", &dims[0], &dims[1], &dims[2], &min_obs, &n_band, &n_free, &seed) != 7) return 2;
    if (ls::fp::fuse_sizes_ok(1, dims[0], dims[1], dims[2]) == false || draw_bad_sizes(1, dims[0], dims[1], dims[2], n_band, n_free) != 0 || min_obs < 1)
        return 3;
    double grid[5];
    for (double& v : grid)
        if (!read_double(&v)) return 2;
    const size_t voxels = (size_t)dims[0] * dims[1] * dims[2];
    std::vector<int> S(voxels), N(voxels);
    for (int& v : S)
        if (scanf("%d", &v) != 1) return 2;
    for (int& v : N)
        if (scanf("%d", &v) != 1) return 2;
    std::vector<long long> list[FIT_KINDS];
    for (size_t i = 0; i < voxels; ++i) list[draw_kind(S[i], N[i], min_obs)].push_back((long long)i);
    const long long cols = n_band + n_free;
    for (long long c = 0; c < cols; ++c) {
        long long j;
        const int kind = draw_column_kind(c, n_band, &j);
        const long long L = (long long)list[kind].size(), T = draw_take(L, kind == FIT_BAND ? n_band : n_free);
        long long index = -1;
        if (j < T) index = list[kind].at((size_t)draw_rank(draw_key(seed, kind), j, L, T));
        float point[3];
        double target;
        unsigned char kd;
        int idx;
        draw_column(index, index >= 0 ? S.at((size_t)index) : 0, index >= 0 ? N.at((size_t)index) : 0, min_obs, dims, grid, grid[3], grid[4], point,
                    &target, &kd, &idx);
        printf("%d %d %a %a %a %a\n", (int)kd, idx, target, (double)point[0], (double)point[1], (double)point[2]);
    }
    printf("%zu %zu %zu\n", list[FIT_BAND].size() + list[FIT_FREE].size(), list[FIT_BAND].size(), list[FIT_FREE].size());
    return 0;
}

static int run_loss() {
    int P, N, has_min;
    if (scanf("%d %d %d", &P, &N, &has_min) != 3 || P < 1 || N < 1) return 2;
    for (int p = 0; p < P; ++p) {
        float s;
        double trunc, min_loss = 0.0;
        if (!read_float(&s) || !read_double(&trunc)) return 2;
        if (has_min && !read_double(&min_loss)) return 2;
        std::vector<int> kind((size_t)N);
        std::vector<float> sdf((size_t)N);
        std::vector<double> target((size_t)N), e2((size_t)N), e((size_t)N);
        long long m = 0;
        for (int i = 0; i < N; ++i) {
            if (scanf("%d", &kind[i]) != 1 || !read_float(&sdf[i]) || !read_double(&target[i])) return 2;
            m += kind[i] != FIT_PAD;
            e[i] = fit_error(kind[i], sdf[i], s, trunc, target[i]);
            e2[i] = e[i] * e[i];
        }
        double total = 0.0;
        for (int c0 = 0; c0 < N; c0 += ls::ts::SAMPLE_CHUNK)
            total += ls::ts::sample_chunk_record(e2.data() + c0, N - c0 < ls::ts::SAMPLE_CHUNK ? N - c0 : ls::ts::SAMPLE_CHUNK, 1);
        const double loss = fit_loss(total, m);
        int improved = 0;
        if (has_min && loss < min_loss) min_loss = loss, improved = 1;
        printf("%a %a %d\n", loss, min_loss, improved);
        for (int i = 0; i < N; ++i) printf("%a%c", (double)fit_grad(e[i], m), i + 1 < N ? ' ' : '\n');
    }
    return 0;
}

int main() {
    char tok[64];
    if (!read_token(tok, sizeof tok)) return 2;
    if (!strcmp(tok, "constants")) {
        printf("%d %d %d %d %d %d %d %d %d %llu\n", FIT_PAD, FIT_BAND, FIT_FREE, DRAW_FIELDS, DRAW_WORD, DRAW_BLOCK_WORDS, DRAW_BLOCK, DRAW_MAX_BLOCKS,
               DRAW_GRID_WORDS, DRAW_GOLDEN);
        return 0;
    }
    if (!strcmp(tok, "draw")) return run_draw();
    if (!strcmp(tok, "loss")) return run_loss();
    return 2;
}

// tsdfray_plan_run.cpp -- csrc/tsdfray_plan.h run on the host: the raycast of a fused state into depth, normal and state images and the
// comparison of a predicted view with an observed one, by the very functions the kernels of csrc/tsdfray.hip loop around.  A stand-alone
// program for tests/test_tsdf_ray_cpu.py, built plain and under AddressSanitizer / UBSan.
//   stdin   "constants";
//           or "cast" nx ny nz min_obs views H W, then origin[3] voxel trunc znear step (hex float64), per view M[12] and K[4] (hex
//           float64), then nx ny nz ints of sum and as many of n;
//           or "compare" count, tol (hex float64), then count rows "d_obs d_pred state" (hex fp32, hex fp32, int)
//   stdout  constants: the constants, the trip bound of (9,8,7) at step 0.25, then the 256 pixels of tile (1, 2) in thread order;
//           cast: per view H W lines "state depth n0 n1 n2" (hex), row-major, then one line of the five counts;
//           compare: count lines of the class, then one line of the five counts
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tsdfray_plan.h"

using namespace ls::tr;

static bool read_token(char* buf, size_t n) { return scanf("%63s", buf) == 1 && n >= 64; }

static bool read_f64(double* v) {
    char tok[64];
    if (!read_token(tok, sizeof tok)) return false;
    *v = strtod(tok, nullptr);
    return true;
}

struct HostFetch {
    const std::vector<int>* S;
    const std::vector<int>* N;
    const int* dims;
    void operator()(const int (&i)[3], int (&s)[8], int (&n)[8]) const {
        const int d[3] = {dims[0], dims[1], dims[2]};
        for (int c = 0; c < 8; ++c) {
            const long long at = ls::ts::sample_corner(d, i, c);
            s[c] = S->at((size_t)at);
            n[c] = N->at((size_t)at);
        }
    }
};

int main() {
    char tok[64];
    if (!read_token(tok, sizeof tok)) return 2;
    if (!strcmp(tok, "constants")) {
        const int dims[3] = {9, 8, 7};
        printf("%d %d %d %d %d %d %lld %lld\n", RAY_STATES, VIEW_CLASSES, RAY_TILE, RAY_WAVE_W, RAY_WAVE_H, RAY_GRID_WORDS, RAY_MAX_TRIPS,
               ray_max_trips(dims, 0.25));
        for (int t = 0; t < RAY_TILE * RAY_TILE; ++t) {
            int px, py;
            ray_pixel(1, 2, t, &px, &py);
            printf("%d %d\n", px, py);
        }
        return 0;
    }
    if (!strcmp(tok, "compare")) {
        long long count;
        double tol;
        if (scanf("%lld", &count) != 1 || count < 0 || !read_f64(&tol)) return 2;
        long long counts[VIEW_CLASSES] = {0, 0, 0, 0, 0};
        for (long long q = 0; q < count; ++q) {
            char a[64], b[64];
            int state;
            if (!read_token(a, sizeof a) || !read_token(b, sizeof b) || scanf("%d", &state) != 1) return 2;
            const int cls = view_class(strtof(a, nullptr), strtof(b, nullptr), state, tol);
            counts[cls] += 1;
            printf("%d\n", cls);
        }
        printf("%lld %lld %lld %lld %lld\n", counts[0], counts[1], counts[2], counts[3], counts[4]);
        return 0;
    }
    if (strcmp(tok, "cast")) return 2;
    int dims[3], min_obs, views, H, W;
    if (scanf("%d %d %d %d %d %d %d", &dims[0], &dims[1], &dims[2], &min_obs, &views, &H, &W) != 7) return 2;
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || views < 0 || H < 1 || W < 1) return 2;
    double grid[7];
    for (double& v : grid)
        if (!read_f64(&v)) return 2;
    std::vector<double> cams((size_t)views * 16);
    for (double& v : cams)
        if (!read_f64(&v)) return 2;
    const size_t voxels = (size_t)dims[0] * dims[1] * dims[2];
    std::vector<int> S(voxels), N(voxels);
    for (int& v : S)
        if (scanf("%d", &v) != 1) return 2;
    for (int& v : N)
        if (scanf("%d", &v) != 1) return 2;
    const double h = grid[3], trunc = grid[4], znear = grid[5], step = grid[6], toh = ls::ts::sample_trunc_over_h(h, trunc);
    if (ls::fp::fuse_bad_grid(grid, h, trunc) || toh != toh || ray_bad_scalar(znear, step)) return 3;
    const HostFetch fetch{&S, &N, dims};
    for (int v = 0; v < views; ++v) {
        const double* M = cams.data() + (size_t)v * 16;
        long long counts[RAY_STATES] = {0, 0, 0, 0, 0};
        for (int py = 0; py < H; ++py)
            for (int px = 0; px < W; ++px) {
                double a[3], b[3];
                float depth, nrm[3];
                ray_setup(M, M + 12, grid, h, px, py, a, b);
                const int st = ray_cast(a, b, dims, znear, step, min_obs, trunc, toh, fetch, &depth, nrm);
                counts[st] += 1;
                printf("%d %a %a %a %a\n", st, (double)depth, (double)nrm[0], (double)nrm[1], (double)nrm[2]);
            }
        printf("%lld %lld %lld %lld %lld\n", counts[0], counts[1], counts[2], counts[3], counts[4]);
    }
    return 0;
}

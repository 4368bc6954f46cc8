// carve_plan_dump -- csrc/carve_plan.h compiled on its own with the host compiler, for tests/test_cloud_carve_cpu.py.
// stdin, one request per line (numbers as C99 hexadecimal doubles, or nan / inf):
//   constants                                                        -> the five states by value, CARVE_MAX_WINDOW, CARVE_CHUNK
//   case W H k empty_is_free tol znear E[12] K[4] x[3] depth[H W]    -> state   (carve_point_view; x and depth are converted to float)
//   drop seen free min_free max_seen                                 -> 0 / 1   (carve_drop)
//   scalars tol znear window min_free max_seen empty_is_free         -> 0, or the number of the first refused argument
//   pieces P a_total n_off_arrays scan_per_block                     -> offs keep pos blk total   (element counts)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "carve_plan.h"

int main() {
    using namespace ls::cp;
    std::string line;
    while (std::getline(std::cin, line)) {
        char* p = line.data();
        if (!strncmp(p, "constants", 9)) {
            printf("%d %d %d %d %d %d %d\n", CARVE_OUT, CARVE_SEEN, CARVE_FREE, CARVE_OCCLUDED, CARVE_MIXED, CARVE_MAX_WINDOW, CARVE_CHUNK);
        } else if (!strncmp(p, "case", 4)) {
            p += 4;
            const int W = (int)strtol(p, &p, 10), H = (int)strtol(p, &p, 10), k = (int)strtol(p, &p, 10), eif = (int)strtol(p, &p, 10);
            const double tol = strtod(p, &p), znear = strtod(p, &p);
            double E[12], K[4];
            float x[3];
            for (double& t : E) t = strtod(p, &p);
            for (double& t : K) t = strtod(p, &p);
            for (float& t : x) t = (float)strtod(p, &p);
            std::vector<float> depth((size_t)W * H);
            for (float& t : depth) t = (float)strtod(p, &p);
            printf("%d\n", carve_point_view(E, K, x, depth.data(), W, H, tol, znear, k, eif != 0));
        } else if (!strncmp(p, "drop", 4)) {
            p += 4;
            int v[4];
            for (int& t : v) t = (int)strtol(p, &p, 10);
            printf("%d\n", carve_drop(v[0], v[1], v[2], v[3]) ? 1 : 0);
        } else if (!strncmp(p, "scalars", 7)) {
            p += 7;
            const double tol = strtod(p, &p), znear = strtod(p, &p);
            int v[4];
            for (int& t : v) t = (int)strtol(p, &p, 10);
            printf("%d\n", carve_bad_scalar(tol, znear, v[0], v[1], v[2], v[3]));
        } else if (!strncmp(p, "pieces", 6)) {
            p += 6;
            const int P = (int)strtol(p, &p, 10);
            const long long a = strtoll(p, &p, 10);
            const int n_off = (int)strtol(p, &p, 10), per = (int)strtol(p, &p, 10);
            const CarvePieces c = carve_pieces(P, a, n_off, per);
            printf("%zu %zu %zu %zu %zu\n", c.offs, c.keep, c.pos, c.blk, c.total);
        } else {
            printf("?\n");
        }
    }
    return 0;
}

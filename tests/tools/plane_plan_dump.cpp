// plane_plan_dump -- csrc/plane_plan.h compiled on its own with the host compiler, for tests/test_depth_plane_cpu.py.
// stdin, one request per line (numbers as C99 hexadecimal doubles, or nan / inf); every request is answered by one line:
//   constants                                             -> the four states, the seven classes, DN_CHUNK, FW_MAX_WEIGHT
//   normals W H max_jump K[4] depth[H W]                  -> per pixel: state n0 n1 n2 (the fp32 normal as a hexadecimal double)   (plane_normal)
//   point d x y K[4]                                      -> P0 P1 P2                                                              (plane_point)
//   fuse W H empty_is_free trunc znear w[4] has_normals E[12] K[4] count x[3 count] depth[H W] (normals[3 H W])
//                                                         -> per position: class q w                                              (plane_voxel_view)
//   update class q w sum n                                -> class sum n                                                           (plane_update)
//   weights w[4]                                          -> -1, or the index of the first refused weight
//   sizes views H W                                       -> 0 / 1                                                                 (plane_sizes_ok)
//   jump max_jump                                         -> 1 if refused
//   pieces views                                          -> the 8-byte words of the normals' workspace
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "plane_plan.h"

int main() {
    using namespace ls::pp;
    std::string line;
    while (std::getline(std::cin, line)) {
        char* p = line.data();
        if (!strncmp(p, "constants", 9)) {
            printf("%d %d %d %d %d %d %d %d %d %d %d %d %d\n", DN_NO_DEPTH, DN_VALID, DN_NO_NEIGHBOUR, DN_DEGENERATE, FW_OUT, FW_EMPTY, FW_OCCLUDED, FW_NEAR_PLANE,
                   FW_NEAR_PROJ, FW_FREE, FW_SATURATED, DN_CHUNK, FW_MAX_WEIGHT);
        } else if (!strncmp(p, "normals", 7)) {
            p += 7;
            const int W = (int)strtol(p, &p, 10), H = (int)strtol(p, &p, 10);
            const double max_jump = strtod(p, &p);
            double K[4];
            for (double& t : K) t = strtod(p, &p);
            std::vector<float> depth((size_t)W * H);
            for (float& t : depth) t = (float)strtod(p, &p);
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    float n[3];
                    const int st = plane_normal(depth.data(), W, H, x, y, K, max_jump, n);
                    printf("%d %a %a %a ", st, (double)n[0], (double)n[1], (double)n[2]);
                }
            printf("\n");
        } else if (!strncmp(p, "point", 5)) {
            p += 5;
            const double d = strtod(p, &p);
            const int x = (int)strtol(p, &p, 10), y = (int)strtol(p, &p, 10);
            double K[4], P[3];
            for (double& t : K) t = strtod(p, &p);
            plane_point(d, x, y, K, P);
            printf("%a %a %a\n", P[0], P[1], P[2]);
        } else if (!strncmp(p, "fuse", 4)) {
            p += 4;
            const int W = (int)strtol(p, &p, 10), H = (int)strtol(p, &p, 10), eif = (int)strtol(p, &p, 10);
            const double trunc = strtod(p, &p), znear = strtod(p, &p);
            int w[4];
            for (int& t : w) t = (int)strtol(p, &p, 10);
            const int has_normals = (int)strtol(p, &p, 10);
            double E[12], K[4];
            for (double& t : E) t = strtod(p, &p);
            for (double& t : K) t = strtod(p, &p);
            const long count = strtol(p, &p, 10);
            std::vector<double> xs((size_t)count * 3);
            for (double& t : xs) t = strtod(p, &p);
            std::vector<float> depth((size_t)W * H), normals(has_normals ? (size_t)W * H * 3 : 0);
            for (float& t : depth) t = (float)strtod(p, &p);
            for (float& t : normals) t = (float)strtod(p, &p);
            for (long i = 0; i < count; ++i) {
                const double x[3] = {xs[(size_t)i * 3], xs[(size_t)i * 3 + 1], xs[(size_t)i * 3 + 2]};
                int q, wt;
                const int cls = plane_voxel_view(E, K, x, depth.data(), has_normals ? normals.data() : nullptr, W, H, trunc, znear, eif != 0, w, &q, &wt);
                printf("%d %d %d ", cls, q, wt);
            }
            printf("\n");
        } else if (!strncmp(p, "update", 6)) {
            p += 6;
            int v[5];
            for (int& t : v) t = (int)strtol(p, &p, 10);
            const int cls = plane_update(v[0], v[1], v[2], &v[3], &v[4]);
            printf("%d %d %d\n", cls, v[3], v[4]);
        } else if (!strncmp(p, "weights", 7)) {
            p += 7;
            int w[4];
            for (int& t : w) t = (int)strtol(p, &p, 10);
            printf("%d\n", plane_bad_weight(w));
        } else if (!strncmp(p, "sizes", 5)) {
            p += 5;
            const long long views = strtoll(p, &p, 10);
            const int H = (int)strtol(p, &p, 10), W = (int)strtol(p, &p, 10);
            printf("%d\n", plane_sizes_ok(views, H, W) ? 1 : 0);
        } else if (!strncmp(p, "jump", 4)) {
            p += 4;
            printf("%d\n", plane_bad_jump(strtod(p, &p)) ? 1 : 0);
        } else if (!strncmp(p, "pieces", 6)) {
            p += 6;
            printf("%zu\n", plane_pieces(strtoll(p, &p, 10)));
        } else {
            printf("?\n");
        }
    }
    return 0;
}

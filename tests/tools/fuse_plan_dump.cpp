// fuse_plan_dump -- csrc/fuse_plan.h compiled on its own with the host compiler, for tests/test_depth_fuse_cpu.py.
// stdin, one request per line (numbers as C99 hexadecimal doubles, or nan / inf); doubles are answered as hexadecimal doubles:
//   constants                                                  -> the six classes by value, FUSE_CHUNK, FUSE_SCALE, FUSE_MAX_OBS, FUSE_GRID_WORDS
//   pos origin h index                                         -> x                  (fuse_position)
//   view W H empty_is_free trunc znear E[12] K[4] x[3] depth[H W] -> class q         (fuse_voxel_view; depth is converted to float)
//   dist depth z trunc empty_is_free                           -> class q            (fuse_distance)
//   update class q sum n                                       -> class sum n        (fuse_update)
//   value sum n min_obs                                        -> valid D            (fuse_value)
//   sizes P nx ny nz                                           -> 0 / 1              (fuse_sizes_ok)
//   grid o0 o1 o2 voxel trunc                                  -> 0, or the number of the first refused field
//   scalars znear empty_is_free                                -> 0, or the number of the first refused argument
//   pieces P                                                   -> offs grids         (8-byte words)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "fuse_plan.h"

int main() {
    using namespace ls::fp;
    std::string line;
    while (std::getline(std::cin, line)) {
        char* p = line.data();
        if (!strncmp(p, "constants", 9)) {
            printf("%d %d %d %d %d %d %d %d %d %d\n", FUSE_OUT, FUSE_EMPTY, FUSE_OCCLUDED, FUSE_NEAR, FUSE_FREE, FUSE_SATURATED, FUSE_CHUNK, FUSE_SCALE,
                   FUSE_MAX_OBS, FUSE_GRID_WORDS);
        } else if (!strncmp(p, "pos", 3)) {
            p += 3;
            const double o = strtod(p, &p), h = strtod(p, &p);
            printf("%a\n", fuse_position(o, h, (int)strtol(p, &p, 10)));
        } else if (!strncmp(p, "view", 4)) {
            p += 4;
            const int W = (int)strtol(p, &p, 10), H = (int)strtol(p, &p, 10), eif = (int)strtol(p, &p, 10);
            const double trunc = strtod(p, &p), znear = strtod(p, &p);
            double E[12], K[4], x[3];
            for (double& t : E) t = strtod(p, &p);
            for (double& t : K) t = strtod(p, &p);
            for (double& t : x) t = strtod(p, &p);
            std::vector<float> depth((size_t)W * H);
            for (float& t : depth) t = (float)strtod(p, &p);
            int q;
            const int cls = fuse_voxel_view(E, K, x, depth.data(), W, H, trunc, znear, eif != 0, &q);
            printf("%d %d\n", cls, q);
        } else if (!strncmp(p, "dist", 4)) {
            p += 4;
            const float d = (float)strtod(p, &p);
            const double z = strtod(p, &p), trunc = strtod(p, &p);
            int q;
            const int cls = fuse_distance(d, z, trunc, strtol(p, &p, 10) != 0, &q);
            printf("%d %d\n", cls, q);
        } else if (!strncmp(p, "update", 6)) {
            p += 6;
            int v[4];
            for (int& t : v) t = (int)strtol(p, &p, 10);
            const int cls = fuse_update(v[0], v[1], &v[2], &v[3]);
            printf("%d %d %d\n", cls, v[2], v[3]);
        } else if (!strncmp(p, "value", 5)) {
            p += 5;
            int v[3];
            for (int& t : v) t = (int)strtol(p, &p, 10);
            bool valid;
            const double D = fuse_value(v[0], v[1], v[2], &valid);
            printf("%d %a\n", valid ? 1 : 0, D);
        } else if (!strncmp(p, "sizes", 5)) {
            p += 5;
            int v[4];
            for (int& t : v) t = (int)strtol(p, &p, 10);
            printf("%d\n", fuse_sizes_ok(v[0], v[1], v[2], v[3]) ? 1 : 0);
        } else if (!strncmp(p, "grid", 4)) {
            p += 4;
            double v[5];
            for (double& t : v) t = strtod(p, &p);
            printf("%d\n", fuse_bad_grid(v, v[3], v[4]));
        } else if (!strncmp(p, "scalars", 7)) {
            p += 7;
            const double znear = strtod(p, &p);
            printf("%d\n", fuse_bad_scalar(znear, (int)strtol(p, &p, 10)));
        } else if (!strncmp(p, "pieces", 6)) {
            p += 6;
            const FusePieces c = fuse_pieces((int)strtol(p, &p, 10));
            printf("%zu %zu\n", c.offs, c.grids);
        } else {
            printf("?\n");
        }
    }
    return 0;
}

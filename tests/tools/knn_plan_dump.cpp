// Replays csrc/knn_plan.h on the host (tests/test_knn_plan_cpu.py): one k-NN build per input line
//   B Nd dst_n Ns C K fma valu_only seeded self has_scratch
// -> one output line: the launches in order as "kernel|grid|block" separated by ';', grid in workgroups, then
// " # enumerator splits tiles_per_split ns_pad tpw stats scratch_bytes used_bytes" (used_bytes: what the planned launches touch of the scratch).
#include <cstdio>
#include "knn_plan.h"

using ls::KnnKernel;

static const char* NAMES[] = {"XYZ_SINGLE", "XYZ_CHUNKED", "SMALL", "TILE", "FUSED_32_T1", "FUSED_32_T2", "FUSED_32_T4", "FUSED_64_T1", "FUSED_64_T2", "FUSED_64_T4"};

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        ls::KnnTraits t;
        int b[5];
        if (sscanf(line, "%d %d %d %d %d %d %d %d %d %d %d", &t.B, &t.Nd, &t.dst_n, &t.Ns, &t.C, &t.K, &b[0], &b[1], &b[2], &b[3], &b[4]) != 11) return 1;
        t.fma = b[0]; t.valu_only = b[1]; t.seeded = b[2]; t.self = b[3]; t.has_scratch = b[4];
        const ls::KnnPlan p = ls::knn_plan(t);
        const char* f = t.fma ? "true" : "false";
        size_t used = 0;
        switch (p.kernel) {
        case KnnKernel::XYZ_SINGLE: case KnnKernel::XYZ_CHUNKED:
            printf("ls::knn_xyz_kernel<%s, %s>|%u|%u", f, p.kernel == KnnKernel::XYZ_SINGLE ? "true" : "false", p.grid, p.block);
            break;
        case KnnKernel::SMALL:
            printf("ls::knn_small_kernel<%s>|%u|%u", f, p.grid, p.block);
            break;
        case KnnKernel::TILE:
            printf("ls::knn_kernel<32, %s>|%u|%u", f, p.grid, p.block);
            if (p.merge_grid) printf(";ls::knn_merge_kernel|%u|256", p.merge_grid);
            used = p.splits > 1 ? (size_t)t.B * t.Nd * p.splits * 16 * 8 : 0;
            break;
        default: {
            const int cc = p.kernel < KnnKernel::FUSED_64_T1 ? 32 : 64;
            for (int s = 0; s < 2; ++s)
                if (p.prep_grid[s]) printf("ls::knn_prep_f16_tile_kernel<%s>|%u|%u;", cc == 32 ? "6, 3" : "12, 4", p.prep_grid[s], p.prep_block);
            printf("ls::knn_fused_kernel<%d, %s, %d>|%u|%u", cc, f, p.tpw, p.grid, p.block);
            used = p.fl.bytes;
        }
        }
        printf(" # %s %d %d %d %d %d %zu %zu\n", NAMES[(int)p.kernel], p.splits, p.tiles_per_split, p.ns_pad, p.tpw, (int)p.stats, p.scratch_bytes, used);
    }
    return 0;
}

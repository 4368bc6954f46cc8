// Replays csrc/edge_plan.h on the host (tests/test_edge_plan_cpu.py): one layer call per input line
//   mode attn Cin Co head_c B Ns Nd has_rows fuse_q fuse_t want_rowmax want_colsum
// (the handle holds the planes the header's two shape predicates allow) -> one output line: the launches in order as "kernel|grid|block" separated
// by ';', grid in workgroups, then " # n_gemm rowmax_parts cs_rows".  A line "limits" prints the unreachable sides of edge_off32_fits instead.
#include <cstdio>
#include <cstring>
#include "edge_plan.h"

using ls::EdgeKernel;

static const char* name(EdgeKernel k) {
    switch (k) {
    case EdgeKernel::POOL: return "ls::edge_pool_kernel";
    case EdgeKernel::POOL_V4_8: return "ls::edge_pool_v4_kernel<8>";
    case EdgeKernel::POOL_V4_16: return "ls::edge_pool_v4_kernel<16>";
    case EdgeKernel::ATTN: return "ls::edge_attn_kernel";
    case EdgeKernel::ATTN_V4_16: return "ls::edge_attn_v4_kernel<16, 1>";
    case EdgeKernel::ATTN_V4_32: return "ls::edge_attn_v4_kernel<32, 1>";
    case EdgeKernel::ATTN_V4_64: return "ls::edge_attn_v4_kernel<64, 1>";
    case EdgeKernel::ATTN_V4_64X2: return "ls::edge_attn_v4_kernel<64, 2>";
    case EdgeKernel::ATTN_FQ_16_32: return "ls::edge_attn_fq_kernel<16, 32>";
    case EdgeKernel::ATTN_FQ_16_64: return "ls::edge_attn_fq_kernel<16, 64>";
    case EdgeKernel::ATTN_FQ_32_64: return "ls::edge_attn_fq_kernel<32, 64>";
    case EdgeKernel::FT_128: return "<128, 128, 1>";
    case EdgeKernel::FT_256: return "<256, 32, 2>";
    }
    return "?";
}

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        if (!strncmp(line, "limits", 6)) {
            // 2^32 bytes of table, 2^24 rows, 2^24 bytes per point, 65536 source points: each held on its own, the other three far away
            printf("%d%d %d%d %d%d %d%d\n", ls::edge_off32_fits(1, 65535, 5461), ls::edge_off32_fits(1, 65535, 5462),     // 65535 * 12 * 5461 < 2^32 <= .. * 5462
                   ls::edge_off32_fits(16384, 1023, 4), ls::edge_off32_fits(16384, 1024, 4), ls::edge_off32_fits(1, 16, 1398101),
                   ls::edge_off32_fits(1, 16, 1398102), ls::edge_off32_fits(1, 65535, 4), ls::edge_off32_fits(1, 65536, 4));
            continue;
        }
        ls::EdgeTraits t;
        int b[7];
        if (sscanf(line, "%d %d %d %d %d %d %d %d %d %d %d %d %d", &t.mode, &b[0], &t.Cin, &t.Co, &t.head_c, &t.B, &t.Ns, &t.Nd, &b[1], &b[2], &b[3], &b[4], &b[5]) != 13) return 1;
        t.attn = b[0]; t.has_rows = b[1]; t.fuse_q = b[2]; t.fuse_t = b[3]; t.want_rowmax = b[4]; t.want_colsum = b[5];
        t.has_wq = t.attn && ls::edge_attn_fq_shape(t.Co, t.Cin, t.head_c);
        t.has_wt = t.attn && ls::edge_ft_shape(t.Co, t.Cin, t.head_c);
        const ls::EdgePlan p = ls::edge_plan(t);
        if (p.kernel == EdgeKernel::FT_128 || p.kernel == EdgeKernel::FT_256) {
            const char* a = name(p.kernel);
            for (int s = 0; s < 2; ++s)
                if (p.prep_grid[s]) printf("ls::edge_ft_prep_a_kernel<%d>|%u|256;", t.Cin / 16, p.prep_grid[s]);
            printf("ls::edge_ft_qk_kernel%s|%u|%u;ls::edge_ft_norms_kernel|%d|256;ls::edge_ft_v_kernel%s|%u|%u", a, p.grid, p.block, t.B, a, p.grid, p.block);
        } else {
            printf("%s|%u|%u", name(p.kernel), p.grid, p.block);
        }
        printf(" # %d %d %d\n", p.n_gemm, p.rowmax_parts, p.cs_rows);
    }
    return 0;
}

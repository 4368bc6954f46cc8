// Replays csrc/gemm_plan.h on the host (tests/test_gemm_plan_cpu.py): one problem per input line
//   mode form M N K lda ldw pieces gather masked may_split latency has_planes wants_out_rowmax C npts has_G_or_cs a_parts has_a_rowmax has_w_rowmax
// (form 0 = gemm_plan, 1 = gemm_vn_plan) -> one output line: the launches as "kernel|grid_x|grid_y|block", separated by ';', grid in workgroups.
#include <cstdio>
#include "gemm_plan.h"

using ls::GemmKernel;

static const char* name(GemmKernel k) {
    switch (k) {
    case GemmKernel::NONE: return "none";
    case GemmKernel::F32_EXACT: return "ls::gemm_f32_kernel<false, 3>";
    case GemmKernel::F32_BF16X3: return "ls::gemm_f32_kernel<true, 3>";
    case GemmKernel::F32_BF16X2: return "ls::gemm_f32_kernel<true, 2>";
    case GemmKernel::F32_F16X2: return "ls::gemm_f32_kernel<true, 22>";
    case GemmKernel::H2: return "ls::gemm_h2_kernel<true, false>";
    case GemmKernel::H2_PLANES: return "ls::gemm_h2_kernel<true, true>";
    case GemmKernel::H2_ANYK: return "ls::gemm_h2_kernel<false, false>";
    case GemmKernel::W2: return "ls::gemm_w2_kernel<false, false>";
    case GemmKernel::W2_PLANES: return "ls::gemm_w2_kernel<false, true>";
    case GemmKernel::W2_MASKED: return "ls::gemm_w2_kernel<true, false>";
    case GemmKernel::W2_MASKED_PLANES: return "ls::gemm_w2_kernel<true, true>";
    case GemmKernel::SMALLK32: return "ls::gemm_smallk_kernel<32, false>";
    case GemmKernel::SMALLK32_GATHER: return "ls::gemm_smallk_kernel<32, true>";
    case GemmKernel::H2_SMALLK32: return "ls::gemm_h2_smallk_kernel<32, false>";
    case GemmKernel::H2_SMALLK32_GATHER: return "ls::gemm_h2_smallk_kernel<32, true>";
    case GemmKernel::H2_SMALLK64: return "ls::gemm_h2_smallk_kernel<64, false>";
    case GemmKernel::H2_SMALLK64_GATHER: return "ls::gemm_h2_smallk_kernel<64, true>";
    case GemmKernel::VN_DIRECT: return "ls::gemm_vn_direct_kernel<64, false>";
    case GemmKernel::VN_DIRECT_ONEPART: return "ls::gemm_vn_direct_kernel<64, true>";
    case GemmKernel::VN_SMALLK32: return "ls::gemm_vn_smallk_kernel<32>";
    case GemmKernel::VN_SMALLK64: return "ls::gemm_vn_smallk_kernel<64>";
    case GemmKernel::VN: return "ls::gemm_vn_kernel<true>";
    case GemmKernel::VN_ANYK: return "ls::gemm_vn_kernel<false>";
    }
    return "?";
}

int main() {
    ls::GemmTraits t;
    int form, b[10];
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &t.mode, &form, &t.M, &t.N, &t.K, &t.lda, &t.ldw, &t.pieces, &b[0], &b[1], &b[2],
                 &b[3], &b[4], &b[5], &t.C, &t.npts, &b[6], &t.a_parts, &b[7], &b[8]) == 20) {
        t.gather = b[0]; t.masked = b[1]; t.may_split = b[2]; t.latency = b[3]; t.has_planes = b[4]; t.wants_out_rowmax = b[5];
        t.has_G_or_cs = b[6]; t.has_a_rowmax = b[7]; t.has_w_rowmax = b[8];
        const ls::GemmPlan p = form ? ls::gemm_vn_plan(t) : ls::gemm_plan(t);
        printf("%s|%u|%u|%u", name(p.kernel), p.grid_x, p.grid_y, p.block);
        if (p.nsplit > 1) printf(";ls::gemm_splitk_reduce_kernel|%u|1|256", p.reduce_grid);
        printf("\n");
    }
    return 0;
}

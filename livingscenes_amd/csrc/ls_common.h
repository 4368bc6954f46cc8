// ls_common.h -- errors, macros, constants and GemmAux for liblivingscenes_hip.so (gfx950 only, wave64).  Device-side helpers: ls_device.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <float.h>
#include <limits.h>

#include "../../include/livingscenes_hip.h"
#include "ls_workspace.h"

namespace ls {

void set_error(const char* fmt, ...);

#define LS_HIP_CHECK(expr)                                                                        \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            ls::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return LS_ERR_HIP;                                                                    \
        }                                                                                         \
    } while (0)

#define LS_REQUIRE(cond, ...)          \
    do {                               \
        if (!(cond)) {                 \
            ls::set_error(__VA_ARGS__); \
            return LS_ERR_INVALID;     \
        }                              \
    } while (0)

#define LS_LAUNCH_CHECK()                                                            \
    do {                                                                             \
        hipError_t _e = hipGetLastError();                                           \
        if (_e != hipSuccess) {                                                      \
            ls::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
            return LS_ERR_HIP;                                                       \
        }                                                                            \
    } while (0)

// Environment: the library reads what ls_model_create documents (LS_ENCODE_GRAPH, LS_SDF_BF16X2) and the process-wide arithmetic mode
// LS_GEMM_MODE (gemm.hip); a library built with -DLS_DEV_KNOBS also reads the race-hunting switches LS_FPS_SIDE and LS_DEBUG_LAYERS (model.hip).
// Latency-bound kernels with one workgroup (or wave) per instance -- FPS, the 32-point k-NN, the heads, matcher, Kabsch -- share their CUs with the chip-filling
// kernels of other steps in flight (and, inside one step, FPS runs beside layers 0 - 1): a raised wave priority makes the SIMD arbiter issue them first.
#ifndef LS_PRIO
#define LS_PRIO 0
#endif
#if LS_PRIO > 0
#define LS_LATENCY_CRITICAL() __builtin_amdgcn_s_setprio(LS_PRIO)
#else
#define LS_LATENCY_CRITICAL()
#endif

constexpr int kWave = 64;
constexpr int kXcds = 8;

// operand range of the f16-split GEMMs (ls_device.h, "operand range of the f16 split"): optional caller-supplied row maxima
struct GemmAux {
    const float* a_rowmax = nullptr;   // [rows of A][a_parts]: max over the parts bounds max|A[row, :]|; indexed by the SOURCE row when a_rows gathers
    int a_parts = 0;
    const float* w_rowmax = nullptr;   // [N]
    const void* w_planes = nullptr;    // pre-split W (gemm_presplit_w_launch): row n = K / 32 lines [hi: 32 f16 | lo: 32 f16] of s_n W[n, :], s_n from w_rowmax (required)
    float* out_rowmax = nullptr;       // [M][2 * cdiv(N, 128)]: max|out[row, 64-column block]| written by the epilogue (un-split launches only)
    const float* cs = nullptr;         // gemm_vn_run only: partial column sums of A ([instance][cs_rows][3][C], edge.hip: attn_colsum) -- the kernel forms the
    int cs_rows = 0;                   // mean part of the conv itself instead of reading G (gemm.hip: gemm_vn_direct_kernel); ignored where that kernel is not taken
};

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// the finaliser of splitmix64: the bit mixer of the bounded hash tables (meshcluster.hip; cloud_grid.h for cloudmerge.hip and cloudnear.hip) and of the counter-based uniforms (meshmetrics.hip)
__host__ __device__ inline unsigned long long mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace ls

// mcubes.hip -- marching cubes on the device, bit-identical (vertex order, face order, float64 coordinates) to the reference's
// vendored PyMCubes:
//   /root/reference/lib_shape_prior/core/models/utils/occnet_utils/utils/libmcubes/marchingcubes.h:23-196   (mc::marching_cubes)
//   /root/reference/lib_shape_prior/core/models/utils/occnet_utils/utils/libmcubes/marchingcubes.cpp:290-326 (interpolation)
// as called on a 3-D array (pywrapper.cpp:90-108) by Generator3D.extract_mesh (occnet_utils/mesh_extractor2.py:161-176).
// SURVEY.md 8 (f-2), second half.
//
// The reference walks the (nx-1)(ny-1)(nz-1) cubes in C order, tests corners with `value <= isovalue`, creates the vertex of
// an edge in the first cube that owns it -- every cube owns its edges 6, 5, 10 (the three meeting at its far corner) and,
// on the low faces of the volume, the otherwise inherited edges -- in the fixed order 6, 5, 10, 0, 1, 2, 3, 4, 7, 8, 9, 11, and
// numbers vertices as they are created.  The sequential numbering is an exclusive prefix sum over per-cube creation counts:
//   count (pattern, #created vertices, #face indices per cube; block sums) -> scan of the block sums -> emit vertices ->
//   emit faces (own vertices by rank, inherited ones from the owning neighbour's base + rank).
// Coordinates carry the library's +0.5 offset (marchingcubes.h:41: lower + dx*i + dx/2), which extract_mesh undoes.
#include "ls_common.h"
#include "ls_scan.h"
#include "mc_tables.h"

namespace ls {

typedef unsigned long long u64;
constexpr int MC_PER_BLOCK = 4096;   // cubes per workgroup of the scan passes (256 threads x 16)

struct McDims { int nx, ny, nz; long long ncubes; int sy, sz; };   // cubes per axis; sample strides of the volume

__constant__ signed char c_tri[256][16];
__constant__ unsigned short c_edge_mask[256];
__constant__ signed char c_tri_len[256];

// creation conditions of the inherited edges on the low faces (marchingcubes.h:96-186)
__device__ __forceinline__ unsigned created_mask(unsigned crossed, int i, int j, int k) {
    const bool i0 = i == 0, j0 = j == 0, k0 = k == 0;
    unsigned m = crossed & ((1u << 6) | (1u << 5) | (1u << 10));
    if (j0 || k0) m |= crossed & (1u << 0);
    if (k0) m |= crossed & ((1u << 1) | (1u << 2));
    if (i0 || k0) m |= crossed & (1u << 3);
    if (j0) m |= crossed & ((1u << 4) | (1u << 9));
    if (i0) m |= crossed & ((1u << 7) | (1u << 11));
    if (i0 || j0) m |= crossed & (1u << 8);
    return m;
}
// rank of edge e among the created edges, in creation order 6, 5, 10, 0, 1, 2, 3, 4, 7, 8, 9, 11
__device__ __forceinline__ int creation_rank(unsigned created, int e) {
    const int order[12] = {6, 5, 10, 0, 1, 2, 3, 4, 7, 8, 9, 11};
    int r = 0;
#pragma unroll
    for (int t = 0; t < 12; ++t) {
        if (order[t] == e) return r;
        r += (created >> order[t]) & 1u;
    }
    return r;
}
__device__ __forceinline__ unsigned cube_pattern(const double* __restrict__ vol, const McDims& d, int i, int j, int k, double iso,
                                                 double (&v)[8]) {
    unsigned cfg = 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        v[m] = vol[((size_t)(i + MC_CX[m]) * d.sy + (j + MC_CY[m])) * d.sz + (k + MC_CZ[m])];
        if (v[m] <= iso) cfg |= 1u << m;
    }
    return cfg;
}

// pass 1: pattern per cube, packed (created vertices << 32 | face indices) summed per workgroup
__global__ __launch_bounds__(256) void mc_count_kernel(const double* __restrict__ vol, McDims d, double iso, unsigned char* __restrict__ cfg_out,
                                                       u64* __restrict__ blk) {
    __shared__ u64 red[4];
    const long long base = (long long)blockIdx.x * MC_PER_BLOCK;
    u64 acc = 0;
    for (int u = 0; u < 16; ++u) {
        const long long c = base + (long long)threadIdx.x * 16 + u;
        if (c >= d.ncubes) break;
        const int k = (int)(c % d.nz), j = (int)((c / d.nz) % d.ny), i = (int)(c / ((long long)d.nz * d.ny));
        double v[8];
        const unsigned cfg = cube_pattern(vol, d, i, j, k, iso, v);
        cfg_out[c] = (unsigned char)cfg;
        const unsigned created = created_mask(c_edge_mask[cfg], i, j, k);
        acc += ((u64)__builtin_popcount(created) << 32) | (u64)c_tri_len[cfg];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// pass 2: exclusive scan of the workgroup sums (one workgroup); totals -> counts_out[0] = vertices, [1] = faces
__global__ __launch_bounds__(1024) void mc_scan_kernel(u64* blk, int nblk, long long* counts_out) {
    const u64 total = scan_top_block<u64>(blk, nblk);
    if (threadIdx.x == 1023) { counts_out[0] = (long long)(total >> 32); counts_out[1] = (long long)(total & 0xFFFFFFFFull) / 3; }
}
// pass 3: per-cube bases (vertex base, face-index base) + the vertices
__global__ __launch_bounds__(256) void mc_vertex_kernel(const double* __restrict__ vol, McDims d, double iso,
                                                        const unsigned char* __restrict__ cfg_in, const u64* __restrict__ blk,
                                                        int* __restrict__ vbase, int* __restrict__ pbase, double* __restrict__ verts,
                                                        long long cap_v) {
#pragma clang fp contract(off)
    __shared__ u64 wsum[4];
    const long long base = (long long)blockIdx.x * MC_PER_BLOCK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u64 mine = 0;
    for (int u = 0; u < 16; ++u) {
        const long long c = base + (long long)tid * 16 + u;
        if (c >= d.ncubes) break;
        const int k = (int)(c % d.nz), j = (int)((c / d.nz) % d.ny), i = (int)(c / ((long long)d.nz * d.ny));
        const unsigned cfg = cfg_in[c];
        mine += ((u64)__builtin_popcount(created_mask(c_edge_mask[cfg], i, j, k)) << 32) | (u64)c_tri_len[cfg];
    }
    u64 inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const u64 v = __shfl_up(inc, o, 64); if (lane >= o) inc += v; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    u64 run = blk[blockIdx.x] + inc - mine;
    for (int w = 0; w < wave; ++w) run += wsum[w];
    for (int u = 0; u < 16; ++u) {
        const long long c = base + (long long)tid * 16 + u;
        if (c >= d.ncubes) break;
        const int k = (int)(c % d.nz), j = (int)((c / d.nz) % d.ny), i = (int)(c / ((long long)d.nz * d.ny));
        const unsigned cfg = cfg_in[c];
        const unsigned created = created_mask(c_edge_mask[cfg], i, j, k);
        const long long vb = (long long)(run >> 32);
        vbase[c] = (int)vb;
        pbase[c] = (int)(run & 0xFFFFFFFFull);
        if (created && verts) {
            double v[8];
            cube_pattern(vol, d, i, j, k, iso, v);
            const int order[12] = {6, 5, 10, 0, 1, 2, 3, 4, 7, 8, 9, 11};
            int r = 0;
#pragma unroll
            for (int t = 0; t < 12; ++t) {
                const int e = order[t];
                if (!((created >> e) & 1u)) continue;
                const int a = MC_EDGE_A[e], b = MC_EDGE_B[e];
                // marchingcubes.h:41-53: sample (i,j,k) sits at i + 0.5; the edge runs from corner a to corner b along one axis
                double p[3] = {(double)(i + MC_CX[a]) + 0.5, (double)(j + MC_CY[a]) + 0.5, (double)(k + MC_CZ[a]) + 0.5};
                const int axis = MC_CX[a] != MC_CX[b] ? 0 : (MC_CY[a] != MC_CY[b] ? 1 : 2);
                const double x1 = p[axis];
                const double x2 = x1 + (double)((axis == 0 ? MC_CX[b] - MC_CX[a] : (axis == 1 ? MC_CY[b] - MC_CY[a] : MC_CZ[b] - MC_CZ[a])));
                const double f1 = v[a], f2 = v[b];
                // marchingcubes.cpp:290-297
                p[axis] = (f2 == f1) ? (x2 + x1) / 2 : (x2 - x1) * (iso - f1) / (f2 - f1) + x1;
                const long long o = vb + r;
                if (o < cap_v) { verts[o * 3 + 0] = p[0]; verts[o * 3 + 1] = p[1]; verts[o * 3 + 2] = p[2]; }
                ++r;
            }
        }
        run += ((u64)__builtin_popcount(created) << 32) | (u64)c_tri_len[cfg];
    }
}
// pass 4: faces
__global__ __launch_bounds__(256) void mc_face_kernel(McDims d, const unsigned char* __restrict__ cfg_in, const int* __restrict__ vbase,
                                                      const int* __restrict__ pbase, long long* __restrict__ faces, long long cap_idx) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= d.ncubes) return;
    const unsigned cfg = cfg_in[c];
    const int len = c_tri_len[cfg];
    if (len == 0) return;
    const int k = (int)(c % d.nz), j = (int)((c / d.nz) % d.ny), i = (int)(c / ((long long)d.nz * d.ny));
    const unsigned created = created_mask(c_edge_mask[cfg], i, j, k);
    // owner of an inherited edge: neighbour cube (i+di, j+dj, k+dk), its edge 6 / 5 / 10   (marchingcubes.h:96-186)
    const signed char odi[12] = {0, 0, 0, -1, 0, 0, 0, -1, -1, 0, 0, -1};
    const signed char odj[12] = {-1, 0, 0, 0, -1, 0, 0, 0, -1, -1, 0, 0};
    const signed char odk[12] = {-1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0};
    const signed char oed[12] = {6, 5, 6, 5, 6, 5, 6, 5, 10, 10, 10, 10};
    const long long pb = pbase[c];
    for (int t = 0; t < len; ++t) {
        const int e = c_tri[cfg][t];
        long long idx;
        if ((created >> e) & 1u) {
            idx = (long long)vbase[c] + creation_rank(created, e);
        } else {
            const int ni = i + odi[e], nj = j + odj[e], nk = k + odk[e];
            const long long nc = ((long long)ni * d.ny + nj) * d.nz + nk;
            const unsigned ncreated = created_mask(c_edge_mask[cfg_in[nc]], ni, nj, nk);
            idx = (long long)vbase[nc] + creation_rank(ncreated, oed[e]);
        }
        if (pb + t < cap_idx) faces[pb + t] = idx;
    }
}

static bool g_mc_tables_ready = false;
static int mc_upload_tables() {
    if (g_mc_tables_ready) return LS_OK;
    unsigned short mask[256];
    signed char len[256];
    for (int cfg = 0; cfg < 256; ++cfg) {
        unsigned m = 0;
        for (int e = 0; e < 12; ++e)
            if (((cfg >> MC_EDGE_A[e]) & 1) != ((cfg >> MC_EDGE_B[e]) & 1)) m |= 1u << e;
        mask[cfg] = (unsigned short)m;
        int l = 0;
        while (l < 16 && MC_TRI_TABLE[cfg][l] >= 0) ++l;
        len[cfg] = (signed char)l;
    }
    LS_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_tri), MC_TRI_TABLE, sizeof(MC_TRI_TABLE)));
    LS_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_edge_mask), mask, sizeof(mask)));
    LS_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_tri_len), len, sizeof(len)));
    g_mc_tables_ready = true;
    return LS_OK;
}

}  // namespace ls

using namespace ls;

extern "C" {

size_t ls_mcubes_workspace_bytes(int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2) return 256;
    const long long nc = (long long)(nx - 1) * (ny - 1) * (nz - 1);
    const long long nblk = (nc + MC_PER_BLOCK - 1) / MC_PER_BLOCK;
    return (size_t)(((nc + 255) & ~255ll) + nc * 8 + 1024 + (nblk + 1) * 8 + 1024);
}

// libmcubes.marching_cubes(volume [nx,ny,nz] float64, isovalue): vertices [nv,3] float64 (with the library's +0.5 offset),
// faces [nf,3] int64.  counts_out (DEVICE long long[2]) = {nv, nf}; call once with vertices = faces = NULL to size the outputs
// (nothing past cap_v vertices / cap_f faces is ever written).  The reference narrows isovalue to float (mcubes.pyx:22): pass
// the narrowed value.
int ls_marching_cubes_f64(const double* volume, int nx, int ny, int nz, double isovalue, double* vertices, long long cap_v,
                          long long* faces, long long cap_f, long long* counts_out, void* workspace, size_t workspace_bytes, void* stream) {
    LS_REQUIRE(volume && counts_out && workspace, "marching_cubes: null argument");
    LS_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "marching_cubes: empty volume");
    LS_REQUIRE((long long)nx * ny * nz < (1ll << 31), "marching_cubes: volume too large");
    hipStream_t st = (hipStream_t)stream;
    if (nx < 2 || ny < 2 || nz < 2) { LS_HIP_CHECK(hipMemsetAsync(counts_out, 0, 16, st)); return LS_OK; }
    if (workspace_bytes < ls_mcubes_workspace_bytes(nx, ny, nz)) { set_error("marching_cubes: workspace too small"); return LS_ERR_WORKSPACE; }
    int rc = mc_upload_tables();
    if (rc != LS_OK) return rc;
    McDims d{nx - 1, ny - 1, nz - 1, (long long)(nx - 1) * (ny - 1) * (nz - 1), ny, nz};
    const int nblk = (int)((d.ncubes + MC_PER_BLOCK - 1) / MC_PER_BLOCK);
    char* ws = (char*)workspace;
    unsigned char* cfg = (unsigned char*)ws;
    size_t off = (size_t)((d.ncubes + 255) & ~255ll);
    int* vbase = (int*)(ws + off); off += (size_t)d.ncubes * 4;
    int* pbase = (int*)(ws + off); off += (size_t)d.ncubes * 4;
    off = (off + 255) & ~(size_t)255;
    u64* blk = (u64*)(ws + off);
    hipLaunchKernelGGL(mc_count_kernel, dim3(nblk), dim3(256), 0, st, volume, d, isovalue, cfg, blk);
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(1024), 0, st, blk, nblk, counts_out);
    hipLaunchKernelGGL(mc_vertex_kernel, dim3(nblk), dim3(256), 0, st, volume, d, isovalue, cfg, blk, vbase, pbase, vertices, cap_v);
    if (faces)
        hipLaunchKernelGGL(mc_face_kernel, dim3(cdiv(d.ncubes, 256)), dim3(256), 0, st, d, cfg, vbase, pbase, faces, cap_f * 3);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

}  // extern "C"

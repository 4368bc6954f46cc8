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

struct McDims { int nx, ny, nz; long long ncubes; int sy, sz; long long samples; };   // cubes per axis; sample strides of the volume; samples per volume

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

// Every kernel below takes a locator by value and asks it which volume its workgroup works on.  The volumes of a batch have one shape and
// lie back to back, and so do their per-cube arrays (cfg, vbase, pbase: [volume][cube]) and the block sums ([volume][block]): volume after
// volume, which is the packed output order, so ONE scan over all block sums numbers the vertices and face indices of the whole batch and
// leaves, at [b][0], where mesh b starts.  The locator of the single op holds nothing: volume 0, known at compile time.
struct OneVolume {
    __device__ int inst() const { return 0; }
    __device__ int count() const { return 1; }
    dim3 grid(int blocks) const { return dim3(blocks); }
};
struct VolumeBatch {
    int B;
    __device__ int inst() const { return blockIdx.y; }
    __device__ int count() const { return B; }
    dim3 grid(int blocks) const { return dim3(blocks, B); }
};
constexpr int MC_MAX_BATCH = 65535;   // gridDim.y

// pass 1: pattern per cube, packed (created vertices << 32 | face indices) summed per workgroup
template <class Vols>
__global__ __launch_bounds__(256) void mc_count_kernel(Vols g, const double* __restrict__ vol, McDims d, double iso, unsigned char* __restrict__ cfg_out,
                                                       u64* __restrict__ blk) {
    __shared__ u64 red[4];
    const int b = g.inst();
    vol += (size_t)b * d.samples;
    cfg_out += (size_t)b * d.ncubes;
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
    if (threadIdx.x == 0) blk[(size_t)b * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// pass 2: exclusive scan of the workgroup sums (one workgroup); the total -> blk[nblk] and, for the single op, counts_out[0] = vertices, [1] = faces
__global__ __launch_bounds__(1024) void mc_scan_kernel(u64* blk, int nblk, long long* counts_out) {
    const u64 total = scan_top_block<u64>(blk, nblk);
    if (threadIdx.x == 1023) {
        blk[nblk] = total;
        if (counts_out) { counts_out[0] = (long long)(total >> 32); counts_out[1] = (long long)(total & 0xFFFFFFFFull) / 3; }
    }
}
// pass 3: per-cube bases (vertex base, face-index base; both count from the start of the packed output) + the vertices; the batch's
// offsets: off_out[b] = first vertex of mesh b, off_out[count + 1 + b] = its first face, [count] / [2 count + 1] = the totals
template <class Vols>
__global__ __launch_bounds__(256) void mc_vertex_kernel(Vols g, const double* __restrict__ vol, McDims d, double iso,
                                                        const unsigned char* __restrict__ cfg_in, const u64* __restrict__ blk,
                                                        int* __restrict__ vbase, int* __restrict__ pbase, double* __restrict__ verts,
                                                        long long cap_v, long long* __restrict__ off_out) {
#pragma clang fp contract(off)
    __shared__ u64 wsum[4];
    const int m = g.inst();
    vol += (size_t)m * d.samples;
    cfg_in += (size_t)m * d.ncubes;
    vbase += (size_t)m * d.ncubes;
    pbase += (size_t)m * d.ncubes;
    const long long base = (long long)blockIdx.x * MC_PER_BLOCK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t first = (size_t)m * gridDim.x;   // the volume's first block sum: where its mesh starts
    if (off_out && blockIdx.x == 0 && tid == 0) {
        const int B = g.count();
        off_out[m] = (long long)(blk[first] >> 32);
        off_out[B + 1 + m] = (long long)(blk[first] & 0xFFFFFFFFull) / 3;
        if (m == B - 1) {
            const u64 total = blk[(size_t)B * gridDim.x];
            off_out[B] = (long long)(total >> 32);
            off_out[2 * B + 1] = (long long)(total & 0xFFFFFFFFull) / 3;
        }
    }
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
    u64 run = blk[first + blockIdx.x] + inc - mine;
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
// pass 4: faces; their vertex indices count from the mesh's own first vertex
template <class Vols>
__global__ __launch_bounds__(256) void mc_face_kernel(Vols g, McDims d, const unsigned char* __restrict__ cfg_in, const int* __restrict__ vbase,
                                                      const int* __restrict__ pbase, const u64* __restrict__ blk, int nblk,
                                                      long long* __restrict__ faces, long long cap_idx) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= d.ncubes) return;
    const int b = g.inst();
    cfg_in += (size_t)b * d.ncubes;
    vbase += (size_t)b * d.ncubes;
    pbase += (size_t)b * d.ncubes;
    const unsigned cfg = cfg_in[c];
    const int len = c_tri_len[cfg];
    if (len == 0) return;
    const long long v0 = (long long)(blk[(size_t)b * nblk] >> 32);
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
        if (pb + t < cap_idx) faces[pb + t] = idx - v0;
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

// per-cube arrays and block sums of B volumes (B = 1: the single op)
struct McWorkspace {
    unsigned char* cfg; int* vbase; int* pbase; u64* blk;
    int nblk;
    size_t total;
};
static McWorkspace mc_workspace(void* workspace, int B, long long ncubes) {
    McWorkspace w{};
    Arena a(workspace);   // null: a sizing pass
    const size_t n = (size_t)B * ncubes;
    w.nblk = (int)((ncubes + MC_PER_BLOCK - 1) / MC_PER_BLOCK);
    w.cfg = a.take<unsigned char>(n);
    w.vbase = a.take<int>(n);
    w.pbase = a.take<int>(n);
    w.blk = a.take<u64>((size_t)B * w.nblk + 1);
    w.total = a.bytes();
    return w;
}

// the launch sequence, written once for both locators
template <class Vols>
static int mc_launch(Vols g, int B, const double* volumes, int nx, int ny, int nz, double isovalue, double* vertices, long long cap_v,
                     long long* faces, long long cap_f, long long* counts_out, long long* off_out, void* workspace, hipStream_t st) {
    int rc = mc_upload_tables();
    if (rc != LS_OK) return rc;
    McDims d{nx - 1, ny - 1, nz - 1, (long long)(nx - 1) * (ny - 1) * (nz - 1), ny, nz, (long long)nx * ny * nz};
    const McWorkspace w = mc_workspace(workspace, B, d.ncubes);
    hipLaunchKernelGGL(mc_count_kernel<Vols>, g.grid(w.nblk), dim3(256), 0, st, g, volumes, d, isovalue, w.cfg, w.blk);
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(1024), 0, st, w.blk, B * w.nblk, counts_out);
    hipLaunchKernelGGL(mc_vertex_kernel<Vols>, g.grid(w.nblk), dim3(256), 0, st, g, volumes, d, isovalue, w.cfg, w.blk, w.vbase, w.pbase, vertices,
                       cap_v, off_out);
    if (faces)
        hipLaunchKernelGGL(mc_face_kernel<Vols>, g.grid(cdiv(d.ncubes, 256)), dim3(256), 0, st, g, d, w.cfg, w.vbase, w.pbase, w.blk, w.nblk, faces,
                           cap_f * 3);
    LS_LAUNCH_CHECK();
    return LS_OK;
}
// vertex and face-index bases are int and share one u64 while they are summed: a cube makes at most 15 face indices, and a mesh has at
// most one vertex per lattice edge (3 per sample)
static bool mc_batch_fits(int B, int nx, int ny, int nz) { return 15ll * B * ((long long)nx * ny * nz) < (1ll << 31); }

}  // namespace ls

using namespace ls;

extern "C" {

size_t ls_mcubes_workspace_bytes(int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2) return 256;
    return mc_workspace(nullptr, 1, (long long)(nx - 1) * (ny - 1) * (nz - 1)).total;
}
size_t ls_mcubes_batch_workspace_bytes(int B, int nx, int ny, int nz) {
    if (B < 1 || B > MC_MAX_BATCH || nx < 1 || ny < 1 || nz < 1 || (long long)nx * ny * nz >= (1ll << 31) || !mc_batch_fits(B, nx, ny, nz)) return 0;
    if (nx < 2 || ny < 2 || nz < 2) return 256;
    return mc_workspace(nullptr, B, (long long)(nx - 1) * (ny - 1) * (nz - 1)).total;
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
    return mc_launch(OneVolume{}, 1, volume, nx, ny, nz, isovalue, vertices, cap_v, faces, cap_f, counts_out, nullptr, workspace, st);
}

// The same for B volumes of one shape, [B,nx,ny,nz]: the meshes packed one after the other, every mesh as ls_marching_cubes_f64 returns
// it (face indices count from the mesh's own first vertex).  off_out (DEVICE long long [2][B+1]): first vertex / first face of every mesh
// and the totals, always the full counts; cap_v / cap_f bound the packed outputs.
int ls_marching_cubes_batch_f64(const double* volumes, int B, int nx, int ny, int nz, double isovalue, double* vertices, long long cap_v,
                                long long* faces, long long cap_f, long long* off_out, void* workspace, size_t workspace_bytes, void* stream) {
    LS_REQUIRE(volumes && off_out && workspace, "marching_cubes_batch: null argument");
    LS_REQUIRE(B >= 1 && B <= MC_MAX_BATCH, "marching_cubes_batch: B=%d outside 1..%d", B, MC_MAX_BATCH);
    LS_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "marching_cubes_batch: empty volume");
    LS_REQUIRE((long long)nx * ny * nz < (1ll << 31), "marching_cubes_batch: volume too large");
    LS_REQUIRE(mc_batch_fits(B, nx, ny, nz), "marching_cubes_batch: 15 * B * nx * ny * nz = 15 * %d * %lld reaches 2^31 (int vertex and face bases)", B,
               (long long)nx * ny * nz);
    LS_REQUIRE(cap_v >= 0 && cap_f >= 0, "marching_cubes_batch: negative capacity");
    hipStream_t st = (hipStream_t)stream;
    if (nx < 2 || ny < 2 || nz < 2) { LS_HIP_CHECK(hipMemsetAsync(off_out, 0, (size_t)(2 * B + 2) * 8, st)); return LS_OK; }
    if (workspace_bytes < ls_mcubes_batch_workspace_bytes(B, nx, ny, nz)) { set_error("marching_cubes_batch: workspace too small"); return LS_ERR_WORKSPACE; }
    return mc_launch(VolumeBatch{B}, B, volumes, nx, ny, nz, isovalue, vertices, cap_v, faces, cap_f, nullptr, off_out, workspace, st);
}

}  // extern "C"

// tsdfmesh_plan.h -- the mesh of a fused state (tsdfmesh.hip), the one statement of it: the pattern of a cube and whether it is kept, the
// edges a cube creates and the ones whose vertex is carried into the mesh, the packed counts of a cube, the position of a vertex and the
// indices of a cube's faces.  Pure functions: no HIP, no global state.  Every kernel of tsdfmesh.hip is a loop around one of them, and
// tests/tools/tsdfmesh_plan_run.cpp runs the SAME functions sequentially on the host, all the way to the vertex and face arrays
// (tests/test_tsdf_mesh_cpu.py holds that program to tests/fuse_oracle.py: mesh by equality).  The definition itself:
// include/livingscenes_hip.h, ls_tsdf_mesh_f64.  Nothing here is shared with mcubes.hip: the creation rules and the owner tables are
// stated again below, host-callable; only the triangle table (mc_tables.h, data) is common.
// Everything is float64 and no a * b + c is contracted into an fma: clang is told here, any other compiler by -ffp-contract=off.
#pragma once
#include <cstddef>

#include "fuse_plan.h"
#include "mc_tables.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ls {
namespace tm {

typedef unsigned long long u64;

enum { MESH_KEPT = 0, MESH_DROPPED_CROSSED, MESH_VALID, MESH_FIELDS };   // stats[p]: kept cubes, dropped cubes that hold a crossing, valid samples
constexpr int MESH_CHUNK = 256;           // threads per workgroup of every pass
constexpr int MESH_ITEMS = 16;            // consecutive cubes per thread of the count and vertex passes
constexpr int MESH_PER_BLOCK = MESH_CHUNK * MESH_ITEMS;   // cubes per workgroup of those passes: 4096
constexpr int MESH_MAX_BATCH = 65535;     // problems per call (the second grid dimension)
constexpr unsigned MESH_KEPT_BIT = 1u << 8;   // of a cube's class: pattern in bits 0 - 7, kept in bit 8

// the order in which a cube creates its vertices, and the owner of an edge the cube does not create: the neighbour cube
// (i + ODI, j + ODJ, k + ODK), as its edge OED (one of 6, 5, 10: the three edges that meet at a cube's far corner)
constexpr signed char MESH_ORDER[12] = {6, 5, 10, 0, 1, 2, 3, 4, 7, 8, 9, 11};
constexpr signed char MESH_ODI[12] = {0, 0, 0, -1, 0, 0, 0, -1, -1, 0, 0, -1};
constexpr signed char MESH_ODJ[12] = {-1, 0, 0, 0, -1, 0, 0, 0, -1, -1, 0, 0};
constexpr signed char MESH_ODK[12] = {-1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0};
constexpr signed char MESH_OED[12] = {6, 5, 6, 5, 6, 5, 6, 5, 10, 10, 10, 10};

// cubes per axis, the sample strides of the state, cubes and samples per problem
struct MeshDims { int cx, cy, cz, sy, sz; long long ncubes, samples; };
LS_CP_HD MeshDims mesh_dims(int nx, int ny, int nz) {
    MeshDims d;
    d.cx = nx - 1; d.cy = ny - 1; d.cz = nz - 1;
    d.sy = ny; d.sz = nz;
    d.ncubes = (long long)(nx - 1) * (long long)(ny - 1) * (long long)(nz - 1);
    d.samples = (long long)nx * (long long)ny * (long long)nz;
    return d;
}
LS_CP_HD long long mesh_blocks(long long ncubes) { return (ncubes + MESH_PER_BLOCK - 1) / MESH_PER_BLOCK; }

// cube c in C order -> (i, j, k); c < 2^31
LS_CP_HD void mesh_cube_ijk(const MeshDims& d, long long c, int* i, int* j, int* k) {
    const unsigned u = (unsigned)c, cz = (unsigned)d.cz, cy = (unsigned)d.cy;
    *k = (int)(u % cz);
    *j = (int)((u / cz) % cy);
    *i = (int)((u / cz) / cy);
}
LS_CP_HD long long mesh_cube_index(const MeshDims& d, int i, int j, int k) { return ((long long)i * d.cy + j) * d.cz + k; }
LS_CP_HD size_t mesh_sample_index(const MeshDims& d, int i, int j, int k) { return ((size_t)i * (size_t)d.sy + (size_t)j) * (size_t)d.sz + (size_t)k; }

// what the sizes of a call may be: P in 1 .. 65535, dims >= 1, 15 P nx ny nz < 2^31 (int vertex and face-index bases that share one
// 64-bit word while they are summed: a cube makes at most 15 face indices, a mesh at most 3 vertices per sample) -> 0, or 1 / 2 / 3
LS_CP_HD int mesh_bad_sizes(int P, int nx, int ny, int nz) {
    if (nx < 1 || ny < 1 || nz < 1) return 1;
    if (P < 1 || P > MESH_MAX_BATCH) return 2;
    const long long lim = 1ll << 31;
    const long long xy = (long long)nx * (long long)ny;                      // < 2^62
    if (xy >= lim) return 3;
    const long long vox = xy * (long long)nz;                                // < 2^62
    if (vox >= lim) return 3;
    return 15ll * (long long)P * vox < lim ? 0 : 3;                          // < 15 * 2^16 * 2^31
}

// the 12-bit mask of the edges whose two corners differ in the pattern
LS_CP_HD unsigned mesh_crossed(unsigned cfg) {
    unsigned m = 0;
    for (int e = 0; e < 12; ++e)
        if (((cfg >> MC_EDGE_A[e]) & 1u) != ((cfg >> MC_EDGE_B[e]) & 1u)) m |= 1u << e;
    return m;
}
// face indices of a pattern: 3 per triangle of its row of the table, at most 15
LS_CP_HD int mesh_tri_len(unsigned cfg) {
    int l = 0;
    while (l < 15 && MC_TRI_TABLE[cfg][l] >= 0) l += 3;
    return l;
}
// the crossed edges cube (i, j, k) creates: always its edges 6, 5, 10 and, on the low faces of the volume, the otherwise inherited ones
LS_CP_HD unsigned mesh_created(unsigned crossed, int i, int j, int k) {
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
// rank of edge e among the edges of `mask`, in creation order
LS_CP_HD int mesh_rank(unsigned mask, int e) {
    int r = 0;
    for (int t = 0; t < 12; ++t) {
        if (MESH_ORDER[t] == e) return r;
        r += (int)((mask >> MESH_ORDER[t]) & 1u);
    }
    return r;
}

// classify: the pattern of cube (i, j, k) from D <= 0 on its eight corners (an invalid corner reads +1: bit clear) and the kept bit: all
// eight corners valid.  sum, n: the state of ONE problem.
LS_CP_HD unsigned mesh_classify(const int* sum, const int* n, const MeshDims& d, int i, int j, int k, int min_obs) {
    unsigned cfg = 0;
    bool kept = true;
    for (int m = 0; m < 8; ++m) {
        const size_t at = mesh_sample_index(d, i + MC_CX[m], j + MC_CY[m], k + MC_CZ[m]);
        bool valid;
        const double D = fp::fuse_value(sum[at], n[at], min_obs, &valid);
        if (D <= 0.0) cfg |= 1u << m;
        kept = kept && valid;
    }
    return cfg | (kept ? MESH_KEPT_BIT : 0u);
}

// The edges of cube (i, j, k) whose vertex is carried into the mesh, given the classes of ONE problem's cubes: the created edges that
// some kept cube names.  A vertex created on a low face (an edge other than 6, 5, 10) is named by its cube alone; the vertex of edge
// 6, 5 or 10 also by the up to three other cubes around that lattice edge, which inherit it:
//   6 (along x): (i, j+1, k+1) as 0, (i, j, k+1) as 2, (i, j+1, k) as 4;   5 (along y): (i, j, k+1) as 1, (i+1, j, k+1) as 3, (i+1, j, k) as 7;
//   10 (along z): (i+1, j+1, k) as 8, (i, j+1, k) as 9, (i+1, j, k) as 11.
// A cube outside the grid is not kept.  Both corners of a carried edge belong to a kept cube, so both are valid samples.
LS_CP_HD bool mesh_kept_at(const unsigned short* cls, const MeshDims& d, int i, int j, int k) {
    if (i >= d.cx || j >= d.cy || k >= d.cz) return false;
    return (cls[mesh_cube_index(d, i, j, k)] & MESH_KEPT_BIT) != 0;
}
LS_CP_HD unsigned mesh_carried(const unsigned short* cls, const MeshDims& d, int i, int j, int k) {
    const unsigned own = cls[mesh_cube_index(d, i, j, k)];
    const unsigned created = mesh_created(mesh_crossed(own & 255u), i, j, k);
    if (own & MESH_KEPT_BIT) return created;
    if (!(created & ((1u << 6) | (1u << 5) | (1u << 10)))) return 0;
    const bool k001 = mesh_kept_at(cls, d, i, j, k + 1), k010 = mesh_kept_at(cls, d, i, j + 1, k), k100 = mesh_kept_at(cls, d, i + 1, j, k);
    unsigned m = 0;
    if (k001 || k010 || mesh_kept_at(cls, d, i, j + 1, k + 1)) m |= 1u << 6;
    if (k001 || k100 || mesh_kept_at(cls, d, i + 1, j, k + 1)) m |= 1u << 5;
    if (k010 || k100 || mesh_kept_at(cls, d, i + 1, j + 1, k)) m |= 1u << 10;
    return created & m;
}

// the packed counts of a cube: (carried vertices << 32) | face indices
LS_CP_HD u64 mesh_counts(unsigned cls, unsigned carried) {
    int bits = 0;
    for (int e = 0; e < 12; ++e) bits += (int)((carried >> e) & 1u);
    return ((u64)bits << 32) | (u64)((cls & MESH_KEPT_BIT) ? mesh_tri_len(cls & 255u) : 0);
}

// the vertex of edge e of cube (i, j, k): the libmcubes interpolation at isovalue 0 between the samples at the edge's two corners, with
// the library's +0.5 offset, then (V - 0.5) * voxel + origin as three separate operations
LS_CP_HD void mesh_vertex(const int* sum, const int* n, const MeshDims& d, int min_obs, const double* origin, double voxel, int i, int j, int k, int e,
                          double (&p)[3]) {
    const int a = MC_EDGE_A[e], b = MC_EDGE_B[e];
    bool valid;
    const size_t at1 = mesh_sample_index(d, i + MC_CX[a], j + MC_CY[a], k + MC_CZ[a]), at2 = mesh_sample_index(d, i + MC_CX[b], j + MC_CY[b], k + MC_CZ[b]);
    const double f1 = fp::fuse_value(sum[at1], n[at1], min_obs, &valid), f2 = fp::fuse_value(sum[at2], n[at2], min_obs, &valid);
    double q[3] = {(double)(i + MC_CX[a]) + 0.5, (double)(j + MC_CY[a]) + 0.5, (double)(k + MC_CZ[a]) + 0.5};
    const int axis = MC_CX[a] != MC_CX[b] ? 0 : (MC_CY[a] != MC_CY[b] ? 1 : 2);
    const int step = axis == 0 ? MC_CX[b] - MC_CX[a] : (axis == 1 ? MC_CY[b] - MC_CY[a] : MC_CZ[b] - MC_CZ[a]);
    const double x1 = q[axis];
    const double x2 = x1 + (double)step;
    q[axis] = (f2 == f1) ? (x2 + x1) / 2 : (x2 - x1) * (0.0 - f1) / (f2 - f1) + x1;
    for (int c = 0; c < 3; ++c) {
        const double shifted = q[c] - 0.5;
        const double scaled = shifted * voxel;
        p[c] = scaled + origin[c];
    }
}

// the carried vertices of cube (i, j, k) in creation order -> vertices[vb ...], nothing at or past cap_v; returns their number
LS_CP_HD int mesh_emit_vertices(const int* sum, const int* n, const MeshDims& d, int min_obs, const double* origin, double voxel, int i, int j, int k,
                                unsigned carried, long long vb, double* vertices, long long cap_v) {
    int r = 0;
    for (int t = 0; t < 12; ++t) {
        const int e = MESH_ORDER[t];
        if (!((carried >> e) & 1u)) continue;
        const long long o = vb + r;
        if (o < cap_v) {
            double p[3];
            mesh_vertex(sum, n, d, min_obs, origin, voxel, i, j, k, e, p);
            vertices[o * 3 + 0] = p[0];
            vertices[o * 3 + 1] = p[1];
            vertices[o * 3 + 2] = p[2];
        }
        ++r;
    }
    return r;
}

// the face indices of the KEPT cube (i, j, k) in table order -> faces[pb ...], nothing at or past cap_idx.  cls, carried, vbase: the
// per-cube arrays of the cube's problem (vbase counts from the start of the packed output, v0 is the problem's first vertex).  A vertex
// the cube creates has its rank among the cube's carried edges (all its created ones: the cube is kept); an inherited one the rank
// of the owner's edge among the OWNER's carried edges.
LS_CP_HD void mesh_emit_faces(const unsigned short* cls, const unsigned short* carried, const int* vbase, const MeshDims& d, int i, int j, int k,
                              long long pb, long long v0, long long* faces, long long cap_idx) {
    const long long c = mesh_cube_index(d, i, j, k);
    const unsigned cfg = cls[c] & 255u;
    const int len = mesh_tri_len(cfg);
    const unsigned created = mesh_created(mesh_crossed(cfg), i, j, k);
    for (int t = 0; t < len; ++t) {
        const int e = MC_TRI_TABLE[cfg][t];
        long long idx;
        if ((created >> e) & 1u) {
            idx = (long long)vbase[c] + mesh_rank(carried[c], e);
        } else {
            const long long oc = mesh_cube_index(d, i + MESH_ODI[e], j + MESH_ODJ[e], k + MESH_ODK[e]);
            idx = (long long)vbase[oc] + mesh_rank(carried[oc], MESH_OED[e]);
        }
        if (pb + t < cap_idx) faces[pb + t] = idx - v0;
    }
}

// the pieces of the workspace, in elements: per cube of the batch the class and the carried mask (16 bit each), the vertex and the
// face-index base (int); per workgroup of the count pass one packed sum, plus the total; P grids of 4 float64 (origin, voxel)
struct MeshPieces { size_t cubes, sums, grid_words; int nblk; };
LS_CP_HD MeshPieces mesh_pieces(int P, int nx, int ny, int nz) {
    const MeshDims d = mesh_dims(nx, ny, nz);
    MeshPieces c;
    c.nblk = (int)mesh_blocks(d.ncubes);
    c.cubes = (size_t)P * (size_t)d.ncubes;
    c.sums = (size_t)P * (size_t)c.nblk + 1;
    c.grid_words = (size_t)P * 4;
    return c;
}

}  // namespace tm
}  // namespace ls

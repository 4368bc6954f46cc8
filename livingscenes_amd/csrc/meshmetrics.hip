// meshmetrics.hip -- the reconstruction metrics of the reference's evaluate.py on one triangle mesh (V [nv,3] float64, F [nf,3] int32):
//   ls_mesh_contains_f64   libmesh.check_mesh_contains (occnet_utils/utils/libmesh/inside_mesh.py:5-154 + triangle_hash.pyx), bit-identical:
//                          the same float64 operations in the same order, and the same 2-D hash (cells of the rescaled (x, y), a triangle in
//                          every cell of its truncated bounding box, a point in the cell of its truncated (x, y)), built on the device
//                          (count, scan, fill) instead of with vector<vector<int>>.  Parity counts do not depend on the order of a cell's list.
//   ls_mesh_distance_f64   |pcu.signed_distance_to_mesh| under a cap (evaluate.py:100-106 only tests |sdf| < thres): closest point on a
//                          triangle per Ericson, Real-Time Collision Detection 5.1.5, over a 3-D grid whose cells are at least max_dist wide;
//                          a triangle is listed in every cell its bounding box grown by max_dist touches, so a point's own cell holds every
//                          triangle closer than max_dist.
//   ls_mesh_sample_f64     trimesh.sample.sample_surface (evaluate.py:25): area-weighted face choice by searchsorted on the cumulative area,
//                          folded barycentric pair; the uniforms come from a counter-based hash (splitmix64) of (seed, 3 i + k).
// The binned ops follow ls_marching_cubes_f64's convention for data-dependent sizes: a call with entries == NULL writes the number of
// bin entries to the device integer count_out and stops; the caller allocates that many and repeats the call.
// ls_mesh_*_batch_f64 run the same kernels on M meshes stored back to back (host int64 offsets, checked on the host and copied to the
// workspace).  Every kernel and every launch sequence is written once, for a mesh locator: with OneMesh a thread's mesh is the call's
// arguments, with RaggedMeshes per-face / per-point kernels find their mesh by binary search of the offsets.  The bounding boxes and the
// sampler's top-level scans run one workgroup per mesh, so the number of launches does not depend on M.  Per mesh the result is bit-identical
// to the single op: contains builds each mesh's own R^2 hash over its own box; distance gives each mesh of a batch a grid of at most a^3
// cells, a^3 <= 8 nf, where the single op takes up to 128^3 (the minimum over a superset of a point's candidate triangles is the same value,
// and its cell still lists every triangle closer than max_dist); the sampler scans each mesh in its own blocks of SCAN_PER_BLOCK faces with
// its own top-level tree.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "ls_common.h"
#include "ls_ragged.h"
#include "ls_scan.h"

// bit-identity with numpy's float64 arithmetic: no contraction of a * b + c into an fma anywhere in this file
#pragma clang fp contract(off)

namespace ls {
namespace mm {

constexpr int DIST_GRID_AXIS = 128;                   // cells per axis of the distance grid at most
constexpr long long DIST_CELLS = (long long)DIST_GRID_AXIS * DIST_GRID_AXIS * DIST_GRID_AXIS;
constexpr int MAX_HASH_RES = 4096;

// per-call parameters the device derives from the mesh (first bytes of every workspace)
struct Params {
    double lo[3], hi[3];        // bounding box of the triangles' corners
    double scale[3], translate[3];
    double org[3], top[3], h[3];   // distance grid: lower / upper end of the domain, cell edge
    int g[3];                   // distance grid: cells per axis
    int valid;                  // contains: finite, non-flat box;  any op: 0 when a face index is out of range
};
constexpr size_t PARAMS_BYTES = 256;
static_assert(sizeof(Params) <= PARAMS_BYTES, "Params");

// ------------------------------------------------------------------------------------------------ which mesh: one, or one of a ragged batch
// Mesh m of a batch owns V[vert_off[m] .. vert_off[m+1]), F[face_off[m] .. face_off[m+1]) (indices local to the mesh) and the points /
// samples [pt_off[m] .. pt_off[m+1]).  The device copy of the offsets (offs) is OFF_ARRAYS arrays of M + 1 int64 back to back; OFF_AUX is
// the mesh's first distance-grid cell (distance) or first scan block (sampler), OFF_AXIS the cells per axis of its distance grid at most.
enum { OFF_V = 0, OFF_F, OFF_P, OFF_AUX, OFF_AXIS, OFF_ARRAYS };

// owner(off, M, i) (ls_ragged.h): the mesh m with off[m] <= i < off[m + 1]; meshes with an empty range are never the owner

// the sampler's key for a seed (mix64: ls_common.h)
__host__ __device__ inline unsigned long long sample_key(unsigned long long seed) { return mix64(seed + 0x9E3779B97F4A7C15ull); }

struct MeshRef {
    const double* V;
    int nv;
    const int32_t* F;
    int nf;
    long long f0;   // global index of the mesh's first face
};

// Every kernel below takes a locator by value and asks it which mesh a face, point, sample or scan block belongs to and where that mesh's
// data starts.  The locator of the single ops holds plain values: no offsets on the device, nothing to upload.
struct OneMesh {
    const double* V;
    int nv;
    const int32_t* F;
    int nf;
    long long n;              // points or samples
    unsigned long long skey;  // sampler: sample_key(seed)
    __device__ long long faces() const { return nf; }
    __device__ long long points() const { return n; }
    __device__ int face_owner(long long) const { return 0; }
    __device__ int point_owner(long long) const { return 0; }
    __device__ int block_owner(long long) const { return 0; }
    __device__ MeshRef mesh(int) const { return {V, nv, F, nf, 0}; }
    __device__ long long aux0(int) const { return 0; }      // first distance-grid cell / first scan block of the mesh
    __device__ int scan_blocks(int) const { return (nf + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK; }
    __device__ long long point0(int) const { return 0; }    // first point / sample of the mesh
    __device__ bool empty(int) const { return false; }      // no faces: the host returned earlier
    __device__ int axis_cap(int) const { return DIST_GRID_AXIS; }
    __device__ unsigned long long key(int) const { return skey; }
};

struct RaggedMeshes {
    const double* V;
    const int32_t* F;
    const long long* offs;    // device copy of the offsets
    int M;
    long long nf_total, n_total;
    const unsigned long long* seeds;   // sampler: device [M]
    __device__ const long long* off(int k) const { return offs + (size_t)k * (M + 1); }
    __device__ long long faces() const { return nf_total; }
    __device__ long long points() const { return n_total; }
    __device__ int face_owner(long long g) const { return owner(off(OFF_F), M, g); }
    __device__ int point_owner(long long i) const { return owner(off(OFF_P), M, i); }
    __device__ int block_owner(long long b) const { return owner(off(OFF_AUX), M, b); }
    __device__ MeshRef mesh(int m) const {
        const long long* vo = off(OFF_V);
        const long long* fo = off(OFF_F);
        return {V + vo[m] * 3, (int)(vo[m + 1] - vo[m]), F + fo[m] * 3, (int)(fo[m + 1] - fo[m]), fo[m]};
    }
    __device__ long long aux0(int m) const { return off(OFF_AUX)[m]; }
    __device__ int scan_blocks(int m) const { return (int)(off(OFF_AUX)[m + 1] - off(OFF_AUX)[m]); }
    __device__ long long point0(int m) const { return off(OFF_P)[m]; }
    __device__ bool empty(int m) const { return off(OFF_F)[m + 1] == off(OFF_F)[m]; }
    __device__ int axis_cap(int m) const { return (int)off(OFF_AXIS)[m]; }
    __device__ unsigned long long key(int m) const { return sample_key(seeds[m]); }
};

// ------------------------------------------------------------------------------------------------ mesh set-up
// corner c of face f; false (and nothing read) when the face refers to a vertex that does not exist
__device__ __forceinline__ bool corner(const double* __restrict__ V, int nv, const int32_t* __restrict__ F, int f, int c, double (&p)[3]) {
    const int vi = F[(size_t)f * 3 + c];
    if ((unsigned)vi >= (unsigned)nv) return false;
    p[0] = V[(size_t)vi * 3 + 0];
    p[1] = V[(size_t)vi * 3 + 1];
    p[2] = V[(size_t)vi * 3 + 2];
    return true;
}

// bounding box of the faces' corners (inside_mesh.py:13-20: unreferenced vertices do not count), the rescaling of the point-in-mesh test
// (scale = (R-1)/(max-min), translate = 0.5 - scale*min) and, for max_dist > 0, the distance grid (at most axis_cap cells per axis).
// One workgroup of 1024 threads.
__device__ void bbox_block(const double* __restrict__ V, int nv, const int32_t* __restrict__ F, int nf, int R, double max_dist, int axis_cap,
                           Params* __restrict__ prm) {
    __shared__ double slo[3][1024], shi[3][1024];
    __shared__ int sbad[1024];
    const int tid = threadIdx.x;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
    for (int f = tid; f < nf; f += 1024)
        for (int c = 0; c < 3; ++c) {
            double p[3];
            if (!corner(V, nv, F, f, c, p)) { bad = 1; continue; }
            for (int a = 0; a < 3; ++a) {
                if (p[a] != p[a]) bad |= 2;   // NaN: numpy's min / max propagate it, every point comes out outside
                lo[a] = fmin(lo[a], p[a]);
                hi[a] = fmax(hi[a], p[a]);
            }
        }
    for (int a = 0; a < 3; ++a) { slo[a][tid] = lo[a]; shi[a][tid] = hi[a]; }
    sbad[tid] = bad;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) {
            for (int a = 0; a < 3; ++a) {
                slo[a][tid] = fmin(slo[a][tid], slo[a][tid + o]);
                shi[a][tid] = fmax(shi[a][tid], shi[a][tid + o]);
            }
            sbad[tid] |= sbad[tid + o];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    int valid = sbad[0] == 0;
    for (int a = 0; a < 3; ++a) {
        const double mn = slo[a][0], mx = shi[a][0];
        prm->lo[a] = mn;
        prm->hi[a] = mx;
        const double sc = (double)(R - 1) / (mx - mn);
        prm->scale[a] = sc;
        prm->translate[a] = 0.5 - sc * mn;
        // a flat mesh: inf / NaN scale in the reference, every rescaled coordinate is inf or NaN and every point fails the box test
        if (!(mx > mn) || !isfinite(sc) || !isfinite(prm->translate[a])) valid = 0;
        if (max_dist > 0) {
            const double org = mn - max_dist, top = mx + max_dist;
            const double cells = (top - org) / max_dist;
            const int g = cells >= (double)axis_cap ? axis_cap : (cells >= 1.0 ? (int)cells : 1);
            prm->org[a] = org;
            prm->top[a] = top;
            prm->g[a] = g;
            prm->h[a] = (top - org) / (double)g;
        }
    }
    prm->valid = sbad[0] & 1 ? -1 : valid;
}

// one workgroup per mesh: prm[m] (max_dist > 0: with its distance grid)
template <class Meshes>
__global__ __launch_bounds__(1024) void bbox_kernel(Meshes L, int R, double max_dist, Params* __restrict__ prm) {
    const int m = blockIdx.x;
    const MeshRef r = L.mesh(m);
    bbox_block(r.V, r.nv, r.F, r.nf, R, max_dist, L.axis_cap(m), prm + m);
}

// ------------------------------------------------------------------------------------------------ point in mesh (inside_mesh.py + triangle_hash.pyx)
struct Cells2 { int x0, x1, y0, y1; };

// <int> of a double as Cython casts it (truncation), clamped to [0, R-1] as triangle_hash.pyx:31-36 does; the argument is clamped to
// [-1, R] first so that the cast is defined for any value
__device__ __forceinline__ int hash_cell(double v, int R) {
    const int i = (int)fmin(fmax(v, -1.0), (double)R);
    return min(max(i, 0), R - 1);
}

__device__ __forceinline__ double rescale(const Params& p, int a, double v) { return p.scale[a] * v + p.translate[a]; }

// face f of a mesh with valid == 1: its rescaled corners (tri_f [9]), its hash cells, their counts
__device__ __forceinline__ void contains_prep_face(const double* __restrict__ V, int nv, const int32_t* __restrict__ F, int f, int R, const Params& p,
                                                   double* __restrict__ tri_f, Cells2* __restrict__ tcell_f, int* __restrict__ cell_count) {
    double t[3][3];
    for (int c = 0; c < 3; ++c) {
        double v[3];
        corner(V, nv, F, f, c, v);   // valid == 1: every index is in range
        for (int a = 0; a < 3; ++a) {
            t[c][a] = rescale(p, a, v[a]);
            tri_f[c * 3 + a] = t[c][a];
        }
    }
    // Cython's min(a, b, c) / max(a, b, c): first operand, replaced by a strictly smaller / larger one
    double mnx = t[0][0], mxx = t[0][0], mny = t[0][1], mxy = t[0][1];
    for (int c = 1; c < 3; ++c) {
        if (t[c][0] < mnx) mnx = t[c][0];
        if (t[c][0] > mxx) mxx = t[c][0];
        if (t[c][1] < mny) mny = t[c][1];
        if (t[c][1] > mxy) mxy = t[c][1];
    }
    const Cells2 cl{hash_cell(mnx, R), hash_cell(mxx, R), hash_cell(mny, R), hash_cell(mxy, R)};
    *tcell_f = cl;
    for (int x = cl.x0; x <= cl.x1; ++x)
        for (int y = cl.y0; y <= cl.y1; ++y) atomicAdd(&cell_count[(size_t)x * R + y], 1);
}

// mesh m's hash is cells [m R^2, (m + 1) R^2); rows of tri / tcell and the bin entries are global face indices
template <class Meshes>
__global__ __launch_bounds__(256) void contains_prep_kernel(Meshes L, int R, const Params* __restrict__ prm, double* __restrict__ tri,
                                                            Cells2* __restrict__ tcell, int* __restrict__ cell_count) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= L.faces()) return;
    const int m = L.face_owner(g);
    if (prm[m].valid != 1) return;
    const Params p = prm[m];
    const MeshRef r = L.mesh(m);
    contains_prep_face(r.V, r.nv, r.F, (int)(g - r.f0), R, p, tri + (size_t)g * 9, tcell + g, cell_count + (size_t)m * R * R);
}

// entries of cell c: entries[start[c] .. start[c] + count[c]); cursor (zeroed) counts the slots taken.  Nothing is written at or past cap.
__device__ __forceinline__ void contains_fill_face(const Cells2 cl, int R, int32_t id, const long long* __restrict__ start, int* __restrict__ cursor,
                                                   int32_t* __restrict__ entries, long long cap) {
    for (int x = cl.x0; x <= cl.x1; ++x)
        for (int y = cl.y0; y <= cl.y1; ++y) {
            const size_t c = (size_t)x * R + y;
            const long long o = start[c] + atomicAdd(&cursor[c], 1);
            if (o < cap) entries[o] = id;
        }
}

template <class Meshes>
__global__ __launch_bounds__(256) void contains_fill_kernel(Meshes L, int R, const Params* __restrict__ prm, const Cells2* __restrict__ tcell,
                                                            const long long* __restrict__ start, int* __restrict__ cursor,
                                                            int32_t* __restrict__ entries, long long cap) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= L.faces()) return;
    const int m = L.face_owner(g);
    if (prm[m].valid != 1) return;
    const size_t base = (size_t)m * R * R;
    contains_fill_face(tcell[g], R, (int32_t)g, start + base, cursor + base, entries, cap);
}

// one point (q [3]) against the triangles of its hash cell: parity of the strict 2-D hits above and below it (inside_mesh.py:39-154).
// The mesh has valid == 1 and its bins are complete; entries index tri in rows of 9.
__device__ bool contains_point(const double* __restrict__ q, int R, const Params& p, const double* __restrict__ tri,
                               const long long* __restrict__ start, const int* __restrict__ count, const int32_t* __restrict__ entries) {
    bool inside = false;
    {
        const double px = rescale(p, 0, q[0]), py = rescale(p, 1, q[1]), pz = rescale(p, 2, q[2]);
        const double Rd = (double)R;
        if (0 <= px && px <= Rd && 0 <= py && py <= Rd && 0 <= pz && pz <= Rd) {
            const int x = (int)px, y = (int)py;      // int(points[i, 0]) (triangle_hash.pyx:58-60); px, py in [0, R]
            if (x < R && y < R) {
                const size_t c = (size_t)x * R + y;
                const long long s = start[c];
                const int m = count[c];
                int n0 = 0, n1 = 0;
                for (int k = 0; k < m; ++k) {
                    const double* t = tri + (size_t)entries[s + k] * 9;
                    const double t0x = t[0], t0y = t[1], t0z = t[2], t1x = t[3], t1y = t[4], t1z = t[5], t2x = t[6], t2y = t[7], t2z = t[8];
                    // check_triangles (:129-154): A = [[t0x - t2x, t1x - t2x], [t0y - t2y, t1y - t2y]], y = p - t2
                    const double a00 = t0x - t2x, a01 = t1x - t2x, a10 = t0y - t2y, a11 = t1y - t2y;
                    const double y0 = px - t2x, y1 = py - t2y;
                    const double det = a00 * a11 - a01 * a10;
                    if (det == 0.0) continue;
                    const double sd = det > 0 ? 1.0 : -1.0, ad = fabs(det);
                    const double u = (a11 * y0 - a01 * y1) * sd;
                    const double v = (-a10 * y0 + a00 * y1) * sd;
                    const double suv = u + v;
                    if (!(0 < u && u < ad && 0 < v && v < ad && 0 < suv && suv < ad)) continue;
                    // compute_intersection_depth (:75-106): normals = np.cross(t3 - t1, t2 - t1) with t1, t2, t3 = corners 0, 1, 2
                    const double v1x = t2x - t0x, v1y = t2y - t0y, v1z = t2z - t0z;
                    const double v2x = t1x - t0x, v2y = t1y - t0y, v2z = t1z - t0z;
                    const double nx = v1y * v2z - v1z * v2y;
                    const double ny = v1z * v2x - v1x * v2z;
                    const double nz = v1x * v2y - v1y * v2x;
                    if (nz == 0.0) continue;                  // NaN depth: counted on neither side
                    const double alpha = nx * (t0x - px) + ny * (t0y - py);
                    const double an = fabs(nz);
                    const double depth = t0z * an + alpha * (nz > 0 ? 1.0 : -1.0);
                    const double pd = pz * an;
                    if (depth >= pd) ++n0;
                    else if (depth < pd) ++n1;
                }
                inside = (n0 & 1) && (n1 & 1);
            }
        }
    }
    return inside;
}

template <class Meshes>
__global__ __launch_bounds__(256) void contains_query_kernel(Meshes L, const double* __restrict__ P, int R, const Params* __restrict__ prm,
                                                             const double* __restrict__ tri, const long long* __restrict__ start,
                                                             const int* __restrict__ count, const int32_t* __restrict__ entries,
                                                             const long long* __restrict__ total, long long cap, uint8_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.points()) return;
    const int m = L.point_owner(i);
    const Params p = prm[m];
    const size_t base = (size_t)m * R * R;
    const bool inside = !L.empty(m) && p.valid == 1 && *total <= cap && contains_point(P + i * 3, R, p, tri, start + base, count + base, entries);
    out[i] = inside ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ distance under a cap
struct Cells3 { int lo[3], hi[3]; };

__device__ __forceinline__ int grid_cell(const Params& p, int a, double v) {
    const double t = floor((v - p.org[a]) / p.h[a]);
    const int i = (int)fmin(fmax(t, -1.0), (double)p.g[a]);
    return min(max(i, 0), p.g[a] - 1);
}

// face f of a mesh with valid >= 0: its corners (tri_f [9]), the grid cells its bounding box grown by max_dist touches, their counts
__device__ __forceinline__ void dist_prep_face(const double* __restrict__ V, int nv, const int32_t* __restrict__ F, int f, double max_dist,
                                               const Params& p, double* __restrict__ tri_f, Cells3* __restrict__ tcell_f, int* __restrict__ cell_count) {
    double t[3][3];
    for (int c = 0; c < 3; ++c) {
        corner(V, nv, F, f, c, t[c]);
        for (int a = 0; a < 3; ++a) tri_f[c * 3 + a] = t[c][a];
    }
    Cells3 cl;
    for (int a = 0; a < 3; ++a) {
        const double mn = fmin(fmin(t[0][a], t[1][a]), t[2][a]), mx = fmax(fmax(t[0][a], t[1][a]), t[2][a]);
        cl.lo[a] = grid_cell(p, a, mn - max_dist);
        cl.hi[a] = grid_cell(p, a, mx + max_dist);
    }
    *tcell_f = cl;
    for (int x = cl.lo[0]; x <= cl.hi[0]; ++x)
        for (int y = cl.lo[1]; y <= cl.hi[1]; ++y)
            for (int z = cl.lo[2]; z <= cl.hi[2]; ++z) atomicAdd(&cell_count[((size_t)x * p.g[1] + y) * p.g[2] + z], 1);
}

// mesh m's grid is the cells from L.aux0(m)
template <class Meshes>
__global__ __launch_bounds__(256) void dist_prep_kernel(Meshes L, double max_dist, const Params* __restrict__ prm, double* __restrict__ tri,
                                                        Cells3* __restrict__ tcell, int* __restrict__ cell_count) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= L.faces()) return;
    const int m = L.face_owner(g);
    if (prm[m].valid < 0) return;
    const Params p = prm[m];
    const MeshRef r = L.mesh(m);
    dist_prep_face(r.V, r.nv, r.F, (int)(g - r.f0), max_dist, p, tri + (size_t)g * 9, tcell + g, cell_count + L.aux0(m));
}

__device__ __forceinline__ void dist_fill_face(const Cells3 cl, int gy, int gz, int32_t id, const long long* __restrict__ start, int* __restrict__ cursor,
                                               int32_t* __restrict__ entries, long long cap) {
    for (int x = cl.lo[0]; x <= cl.hi[0]; ++x)
        for (int y = cl.lo[1]; y <= cl.hi[1]; ++y)
            for (int z = cl.lo[2]; z <= cl.hi[2]; ++z) {
                const size_t c = ((size_t)x * gy + y) * gz + z;
                const long long o = start[c] + atomicAdd(&cursor[c], 1);
                if (o < cap) entries[o] = id;
            }
}

template <class Meshes>
__global__ __launch_bounds__(256) void dist_fill_kernel(Meshes L, const Params* __restrict__ prm, const Cells3* __restrict__ tcell,
                                                        const long long* __restrict__ start, int* __restrict__ cursor, int32_t* __restrict__ entries,
                                                        long long cap) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= L.faces()) return;
    const int m = L.face_owner(g);
    if (prm[m].valid < 0) return;
    const long long base = L.aux0(m);
    dist_fill_face(tcell[g], prm[m].g[1], prm[m].g[2], (int32_t)g, start + base, cursor + base, entries, cap);
}

__device__ __forceinline__ double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ double d2_at(const double* p, const double* a, const double* d, double s) {   // |p - (a + s d)|^2
    double r = 0;
    for (int k = 0; k < 3; ++k) {
        const double e = p[k] - (a[k] + s * d[k]);
        r += e * e;
    }
    return r;
}
__device__ __forceinline__ double seg_d2(const double* p, const double* a, const double* b) {
    double ab[3], ap[3];
    for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ap[k] = p[k] - a[k]; }
    const double l = dot3(ab, ab);
    double s = l > 0 ? dot3(ap, ab) / l : 0.0;
    s = fmin(fmax(s, 0.0), 1.0);
    return d2_at(p, a, ab, s);
}

// squared distance from p to triangle (a, b, c): Ericson, Real-Time Collision Detection 5.1.5 (ClosestPtPointTriangle); a triangle of zero
// area that reaches the face region is the nearest of its three edges (segments, or points when they collapse)
__device__ double point_triangle_d2(const double* p, const double* a, const double* b, const double* c) {
    double ab[3], ac[3], ap[3], bp[3], cp[3];
    for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = p[k] - a[k]; bp[k] = p[k] - b[k]; cp[k] = p[k] - c[k]; }
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    if (d1 <= 0 && d2 <= 0) return dot3(ap, ap);
    const double d3 = dot3(ab, bp), d4 = dot3(ac, bp);
    if (d3 >= 0 && d4 <= d3) return dot3(bp, bp);
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0 && d1 >= 0 && d3 <= 0) {
        const double den = d1 - d3;
        return d2_at(p, a, ab, den > 0 ? d1 / den : 0.0);
    }
    const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    if (d6 >= 0 && d5 <= d6) return dot3(cp, cp);
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0 && d2 >= 0 && d6 <= 0) {
        const double den = d2 - d6;
        return d2_at(p, a, ac, den > 0 ? d2 / den : 0.0);
    }
    const double va = d3 * d6 - d5 * d4;
    const double e43 = d4 - d3, e56 = d5 - d6;
    if (va <= 0 && e43 >= 0 && e56 >= 0) {
        double bc[3];
        for (int k = 0; k < 3; ++k) bc[k] = c[k] - b[k];
        const double den = e43 + e56;
        return d2_at(p, b, bc, den > 0 ? e43 / den : 0.0);
    }
    const double den = va + vb + vc;
    if (!(den > 0)) return fmin(fmin(seg_d2(p, a, b), seg_d2(p, b, c)), seg_d2(p, c, a));
    const double v = vb / den, w = vc / den;
    double r = 0;
    for (int k = 0; k < 3; ++k) {
        const double e = p[k] - (a[k] + ab[k] * v + ac[k] * w);
        r += e * e;
    }
    return r;
}

// distance from q [3] to the mesh when < max_dist, +inf otherwise; binned = the mesh's bins are complete (valid >= 0, nothing past cap)
__device__ double dist_point(const double* __restrict__ P3, double max_dist, const Params& p, bool binned, const double* __restrict__ tri,
                             const long long* __restrict__ start, const int* __restrict__ count, const int32_t* __restrict__ entries) {
    double best = INFINITY;
    const double q[3] = {P3[0], P3[1], P3[2]};
    // outside [min - max_dist, max + max_dist] on an axis: farther than max_dist from every triangle
    const bool in_dom = q[0] >= p.org[0] && q[0] <= p.top[0] && q[1] >= p.org[1] && q[1] <= p.top[1] && q[2] >= p.org[2] && q[2] <= p.top[2];
    if (binned && in_dom) {
        const size_t c = ((size_t)grid_cell(p, 0, q[0]) * p.g[1] + grid_cell(p, 1, q[1])) * p.g[2] + grid_cell(p, 2, q[2]);
        const long long s = start[c];
        const int m = count[c];
        for (int k = 0; k < m; ++k) {
            const double* t = tri + (size_t)entries[s + k] * 9;
            best = fmin(best, point_triangle_d2(q, t, t + 3, t + 6));
        }
    }
    const double d = sqrt(best);
    return d < max_dist ? d : INFINITY;
}

template <class Meshes>
__global__ __launch_bounds__(256) void dist_query_kernel(Meshes L, const double* __restrict__ P, double max_dist, const Params* __restrict__ prm,
                                                         const double* __restrict__ tri, const long long* __restrict__ start,
                                                         const int* __restrict__ count, const int32_t* __restrict__ entries,
                                                         const long long* __restrict__ total, long long cap, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.points()) return;
    const int m = L.point_owner(i);
    if (L.empty(m)) { out[i] = INFINITY; return; }   // an empty mesh is infinitely far away
    const Params p = prm[m];
    const long long base = L.aux0(m);
    out[i] = dist_point(P + i * 3, max_dist, p, p.valid >= 0 && *total <= cap, tri, start + base, count + base, entries);
}

__global__ __launch_bounds__(256) void fill_f64_kernel(double* __restrict__ out, long long n, double v) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = v;
}

// ------------------------------------------------------------------------------------------------ surface sampling (trimesh.sample.sample_surface)
// uniform in [0, 1): the top 53 bits of splitmix64's output for counter j of the stream with key sample_key(seed)
__device__ __forceinline__ double uniform(unsigned long long key, unsigned long long j) {
    return (double)(mix64(key + (j + 1ull) * 0x9E3779B97F4A7C15ull) >> 11) * 0x1.0p-53;
}

// trimesh Trimesh.area_faces: |cross(v1 - v0, v2 - v0)| / 2, components written as np.cross does
__device__ __forceinline__ double face_area(const double* __restrict__ V, int nv, const int32_t* __restrict__ F, int f) {
    double a[3], b[3], c[3];
    if (!corner(V, nv, F, f, 0, a) || !corner(V, nv, F, f, 1, b) || !corner(V, nv, F, f, 2, c)) return 0.0;
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const double wx = c[0] - a[0], wy = c[1] - a[1], wz = c[2] - a[2];
    const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
    return sqrt(cx * cx + cy * cy + cz * cz) / 2.0;
}

template <class Meshes>
__global__ __launch_bounds__(256) void area_kernel(Meshes L, double* __restrict__ area) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= L.faces()) return;
    const MeshRef r = L.mesh(L.face_owner(g));
    area[g] = face_area(r.V, r.nv, r.F, (int)(g - r.f0));
}

// each mesh's inclusive scan of its face areas: its own blocks of SCAN_PER_BLOCK faces (block sums blk[L.aux0(m) ...]), then one top-level
// workgroup per mesh, then the prefixes -- the three steps of scan() above, per mesh
template <class Meshes>
__global__ __launch_bounds__(SCAN_T) void area_scan_reduce_kernel(Meshes L, const double* __restrict__ area, double* __restrict__ blk) {
    const int m = L.block_owner(blockIdx.x);
    const MeshRef r = L.mesh(m);
    scan_reduce_block<double, double>(area + r.f0, r.nf, blockIdx.x - L.aux0(m), blk + blockIdx.x);
}

template <class Meshes>
__global__ __launch_bounds__(1024) void area_scan_top_kernel(Meshes L, double* __restrict__ blk) {
    const int m = blockIdx.x;
    const int nblk = L.scan_blocks(m);
    if (nblk == 0) return;   // a mesh nobody samples
    scan_top_block<double>(blk + L.aux0(m), nblk);
}

template <class Meshes>
__global__ __launch_bounds__(SCAN_T) void area_scan_apply_kernel(Meshes L, const double* __restrict__ area, const double* __restrict__ blk,
                                                                 double* __restrict__ cum) {
    const int m = L.block_owner(blockIdx.x);
    const MeshRef r = L.mesh(m);
    scan_apply_block<double, double, true>(area + r.f0, r.nf, blockIdx.x - L.aux0(m), blk[blockIdx.x], cum + r.f0);
}

// sample i of a mesh (cum: its inclusive cumulative face areas): point pts3 [3], local face index *face_i (face_i nullable)
__device__ __forceinline__ void sample_one(const double* __restrict__ V, int nv, const int32_t* __restrict__ F, int nf, const double* __restrict__ cum,
                                           unsigned long long key, long long i, double* __restrict__ pts3, int64_t* __restrict__ face_i) {
    const unsigned long long j = 3ull * (unsigned long long)i;
    const double pick = uniform(key, j) * cum[nf - 1];
    // np.searchsorted(cumsum, pick) (side 'left'): first face whose cumulative area reaches pick
    int lo = 0, hi = nf - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (cum[mid] >= pick) hi = mid;
        else lo = mid + 1;
    }
    double r1 = uniform(key, j + 1), r2 = uniform(key, j + 2);
    if (r1 + r2 > 1.0) { r1 = fabs(r1 - 1.0); r2 = fabs(r2 - 1.0); }
    double a[3] = {0, 0, 0}, b[3] = {0, 0, 0}, c[3] = {0, 0, 0};
    const bool ok = corner(V, nv, F, lo, 0, a) && corner(V, nv, F, lo, 1, b) && corner(V, nv, F, lo, 2, c);
    for (int k = 0; k < 3; ++k)   // (tri_vectors * random_lengths).sum(axis=1) + tri_origins
        pts3[k] = ok ? (r1 * (b[k] - a[k]) + r2 * (c[k] - a[k])) + a[k] : NAN;
    if (face_i) *face_i = lo;
}

template <class Meshes>
__global__ __launch_bounds__(256) void sample_kernel(Meshes L, const double* __restrict__ cum, double* __restrict__ pts,
                                                     int64_t* __restrict__ face_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.points()) return;
    const int m = L.point_owner(i);
    const MeshRef r = L.mesh(m);
    sample_one(r.V, r.nv, r.F, r.nf, cum + r.f0, L.key(m), i - L.point0(m), pts + i * 3, face_out ? face_out + i : nullptr);
}

}  // namespace mm
}  // namespace ls

using namespace ls;
using namespace ls::mm;

namespace {
struct BinWs {
    long long* offs;   // a batch: the device copy of the offsets
    Params* prm;       // [M]
    double* tri;
    void* tcell;
    int* cell_count;
    long long* start;
    long long* blk;
    size_t bytes;      // of the whole layout
};
// ws null: a sizing pass.  n_offs: OFF_ARRAYS * (M + 1) for a batch, 0 (no bytes) for one mesh
BinWs bin_layout(void* ws, size_t n_offs, int M, long long nf, long long cells, size_t cell_rec) {
    Arena a(ws);
    BinWs w;
    w.offs = a.take<long long>(n_offs);
    w.prm = a.take<Params>((size_t)M);
    w.tri = a.take<double>((size_t)nf * 9);
    w.tcell = a.take<char>((size_t)nf * cell_rec);
    w.cell_count = a.take<int>((size_t)cells);
    w.start = a.take<long long>((size_t)cells);
    w.blk = a.take<long long>((size_t)scan_blocks(cells));
    w.bytes = a.bytes();
    return w;
}
struct SampleWs {
    long long* offs;
    double* area;
    double* cum;
    double* blk;
    size_t bytes;
};
SampleWs sample_layout(void* ws, size_t n_offs, long long nf, long long nblk) {
    Arena a(ws);
    SampleWs w;
    w.offs = a.take<long long>(n_offs);
    w.area = a.take<double>((size_t)nf);
    w.cum = a.take<double>((size_t)nf);
    w.blk = a.take<double>((size_t)nblk);
    w.bytes = a.bytes();
    return w;
}
size_t n_offs(int M) { return (size_t)OFF_ARRAYS * (M + 1); }

// ---- the launch sequences, one per metric: M meshes located by L, nf faces and n points (samples) in all, w the carved workspace
template <class Meshes>
int contains_launch(const Meshes& L, int M, long long nf, const double* points, long long n, int R, const BinWs& w, uint8_t* inside_out,
                    int32_t* entries, long long cap_entries, long long* count_out, hipStream_t st) {
    const long long cells = (long long)M * R * R;
    Cells2* tcell = (Cells2*)w.tcell;
    const int fb = cdiv(nf, 256);
    LS_HIP_CHECK(hipMemsetAsync(w.cell_count, 0, (size_t)cells * sizeof(int), st));
    hipLaunchKernelGGL(bbox_kernel<Meshes>, dim3(M), dim3(1024), 0, st, L, R, 0.0, w.prm);
    hipLaunchKernelGGL(contains_prep_kernel<Meshes>, dim3(fb), dim3(256), 0, st, L, R, w.prm, w.tri, tcell, w.cell_count);
    scan<int, long long, false>(w.cell_count, cells, w.blk, w.start, count_out, st);
    LS_LAUNCH_CHECK();
    if (!entries) return LS_OK;   // sizing call: one entry count for all the meshes
    // the fill takes its slots with a zeroed cursor in cell_count, which ends equal to the counts the query reads
    LS_HIP_CHECK(hipMemsetAsync(w.cell_count, 0, (size_t)cells * sizeof(int), st));
    hipLaunchKernelGGL(contains_fill_kernel<Meshes>, dim3(fb), dim3(256), 0, st, L, R, w.prm, tcell, w.start, w.cell_count, entries, cap_entries);
    if (n > 0)
        hipLaunchKernelGGL(contains_query_kernel<Meshes>, dim3(cdiv(n, 256)), dim3(256), 0, st, L, points, R, w.prm, w.tri, w.start, w.cell_count,
                           entries, count_out, cap_entries, inside_out);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

template <class Meshes>
int distance_launch(const Meshes& L, int M, long long nf, const double* points, long long n, double max_dist, long long cells, const BinWs& w,
                    double* dist_out, int32_t* entries, long long cap_entries, long long* count_out, hipStream_t st) {
    Cells3* tcell = (Cells3*)w.tcell;
    const int fb = cdiv(nf, 256);
    LS_HIP_CHECK(hipMemsetAsync(w.cell_count, 0, (size_t)cells * sizeof(int), st));
    hipLaunchKernelGGL(bbox_kernel<Meshes>, dim3(M), dim3(1024), 0, st, L, 2, max_dist, w.prm);
    hipLaunchKernelGGL(dist_prep_kernel<Meshes>, dim3(fb), dim3(256), 0, st, L, max_dist, w.prm, w.tri, tcell, w.cell_count);
    scan<int, long long, false>(w.cell_count, cells, w.blk, w.start, count_out, st);
    LS_LAUNCH_CHECK();
    if (!entries) return LS_OK;
    LS_HIP_CHECK(hipMemsetAsync(w.cell_count, 0, (size_t)cells * sizeof(int), st));
    hipLaunchKernelGGL(dist_fill_kernel<Meshes>, dim3(fb), dim3(256), 0, st, L, w.prm, tcell, w.start, w.cell_count, entries, cap_entries);
    if (n > 0)
        hipLaunchKernelGGL(dist_query_kernel<Meshes>, dim3(cdiv(n, 256)), dim3(256), 0, st, L, points, max_dist, w.prm, w.tri, w.start,
                           w.cell_count, entries, count_out, cap_entries, dist_out);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

// nblk scan blocks in all (> 0: some mesh is sampled, and it has faces)
template <class Meshes>
int sample_launch(const Meshes& L, int M, long long nf, int nblk, long long count, const SampleWs& w, double* points_out, int64_t* face_out,
                  hipStream_t st) {
    hipLaunchKernelGGL(area_kernel<Meshes>, dim3(cdiv(nf, 256)), dim3(256), 0, st, L, w.area);
    hipLaunchKernelGGL(area_scan_reduce_kernel<Meshes>, dim3(nblk), dim3(SCAN_T), 0, st, L, w.area, w.blk);
    hipLaunchKernelGGL(area_scan_top_kernel<Meshes>, dim3(M), dim3(1024), 0, st, L, w.blk);
    hipLaunchKernelGGL(area_scan_apply_kernel<Meshes>, dim3(nblk), dim3(SCAN_T), 0, st, L, w.area, w.blk, w.cum);
    hipLaunchKernelGGL(sample_kernel<Meshes>, dim3(cdiv(count, 256)), dim3(256), 0, st, L, w.cum, points_out, face_out);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

// off[0] = 0, never decreasing, at most per_max per mesh, ending at total
int check_ranges(const char* op, const char* what, int M, const long long* off, long long total, long long per_max) {
    return ls::check_ranges(op, "mesh", what, M, off, total, per_max);
}

// the argument checks of the single-mesh ops, per mesh
int check_meshes(const char* op, int M, const double* V, long long nv_total, const long long* vert_off, const int32_t* F, long long nf_total,
                 const long long* face_off) {
    LS_REQUIRE(M >= 0 && nv_total >= 0 && nf_total >= 0, "%s: negative size (M %d, nv_total %lld, nf_total %lld)", op, M, nv_total, nf_total);
    LS_REQUIRE(nf_total <= INT_MAX, "%s: %lld faces in the batch, at most %d", op, nf_total, INT_MAX);
    int rc = check_ranges(op, "vert_off", M, vert_off, nv_total, INT_MAX);
    if (rc != LS_OK) return rc;
    rc = check_ranges(op, "face_off", M, face_off, nf_total, INT_MAX);
    if (rc != LS_OK) return rc;
    for (int m = 0; m < M; ++m)
        LS_REQUIRE(face_off[m + 1] == face_off[m] || vert_off[m + 1] > vert_off[m], "%s: mesh %d: %lld faces and no vertices", op, m,
                   face_off[m + 1] - face_off[m]);
    LS_REQUIRE(nf_total == 0 || (V && F), "%s: null vertices / faces with nf_total = %lld", op, nf_total);
    return LS_OK;
}

// the device copy of the offsets (aux, axis: nullable, zeros), in the order of OFF_*
std::vector<long long> pack_offsets(int M, const long long* vert_off, const long long* face_off, const long long* pt_off, const long long* aux,
                                    const long long* axis) {
    return ls::pack_offsets(M, {vert_off, face_off, pt_off, aux, axis});
}

// cells per axis of a mesh's distance grid in a batch: the largest a <= DIST_GRID_AXIS with a^3 <= 8 nf, at least 1 -- so the grids of
// a batch hold at most 8 nf_total + M cells, where the single op always takes 128^3
long long dist_axis_cap(long long nf) {
    const long long t = 8 * nf;
    long long a = (long long)std::cbrt((double)t);
    while (a > 1 && a * a * a > t) --a;
    while ((a + 1) * (a + 1) * (a + 1) <= t) ++a;
    return std::min<long long>(std::max<long long>(a, 1), DIST_GRID_AXIS);
}
}  // namespace

extern "C" {

size_t ls_mesh_contains_workspace_bytes(int nf, int hash_resolution) {
    if (nf < 0 || hash_resolution < 2 || hash_resolution > MAX_HASH_RES) return 0;
    return bin_layout(nullptr, 0, 1, nf, (long long)hash_resolution * hash_resolution, sizeof(Cells2)).bytes;
}

int ls_mesh_contains_f64(const double* vertices, int nv, const int32_t* faces, int nf, const double* points, long long n, int hash_resolution,
                         uint8_t* inside_out, int32_t* entries, long long cap_entries, long long* count_out, void* workspace,
                         size_t workspace_bytes, void* stream) {
    LS_REQUIRE(nf >= 0 && nv >= 0 && n >= 0, "mesh_contains: negative size (nv %d, nf %d, n %lld)", nv, nf, n);
    LS_REQUIRE(hash_resolution >= 2 && hash_resolution <= MAX_HASH_RES, "mesh_contains: hash_resolution must be in [2, %d], got %d",
               MAX_HASH_RES, hash_resolution);
    LS_REQUIRE(nf == 0 || (vertices && faces && nv > 0), "mesh_contains: null vertices / faces with nf = %d", nf);
    LS_REQUIRE(count_out, "mesh_contains: null count_out");
    LS_REQUIRE(cap_entries >= 0, "mesh_contains: negative cap_entries");
    LS_REQUIRE(!entries || n == 0 || (points && inside_out), "mesh_contains: null points / inside_out with n = %lld", n);
    hipStream_t st = (hipStream_t)stream;
    if (nf == 0) {   // an empty mesh contains nothing
        LS_HIP_CHECK(hipMemsetAsync(count_out, 0, sizeof(long long), st));
        if (entries && n > 0) LS_HIP_CHECK(hipMemsetAsync(inside_out, 0, (size_t)n, st));
        return LS_OK;
    }
    const int R = hash_resolution;
    if (!workspace || workspace_bytes < ls_mesh_contains_workspace_bytes(nf, R)) {
        set_error("mesh_contains: workspace too small (need ls_mesh_contains_workspace_bytes(%d, %d))", nf, R);
        return LS_ERR_WORKSPACE;
    }
    const BinWs w = bin_layout(workspace, 0, 1, nf, (long long)R * R, sizeof(Cells2));
    return contains_launch(OneMesh{vertices, nv, faces, nf, n, 0}, 1, nf, points, n, R, w, inside_out, entries, cap_entries, count_out, st);
}

size_t ls_mesh_distance_workspace_bytes(int nf) {
    if (nf < 0) return 0;
    return bin_layout(nullptr, 0, 1, nf, DIST_CELLS, sizeof(Cells3)).bytes;
}

int ls_mesh_distance_f64(const double* vertices, int nv, const int32_t* faces, int nf, const double* points, long long n, double max_dist,
                         double* dist_out, int32_t* entries, long long cap_entries, long long* count_out, void* workspace,
                         size_t workspace_bytes, void* stream) {
    LS_REQUIRE(nf >= 0 && nv >= 0 && n >= 0, "mesh_distance: negative size (nv %d, nf %d, n %lld)", nv, nf, n);
    LS_REQUIRE(max_dist > 0 && max_dist < (double)INFINITY, "mesh_distance: max_dist must be positive and finite, got %g", max_dist);
    LS_REQUIRE(nf == 0 || (vertices && faces && nv > 0), "mesh_distance: null vertices / faces with nf = %d", nf);
    LS_REQUIRE(count_out, "mesh_distance: null count_out");
    LS_REQUIRE(cap_entries >= 0, "mesh_distance: negative cap_entries");
    LS_REQUIRE(!entries || n == 0 || (points && dist_out), "mesh_distance: null points / dist_out with n = %lld", n);
    hipStream_t st = (hipStream_t)stream;
    if (nf == 0) {   // an empty mesh is infinitely far away
        LS_HIP_CHECK(hipMemsetAsync(count_out, 0, sizeof(long long), st));
        if (entries && n > 0) hipLaunchKernelGGL(fill_f64_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, dist_out, n, (double)INFINITY);
        LS_LAUNCH_CHECK();
        return LS_OK;
    }
    if (!workspace || workspace_bytes < ls_mesh_distance_workspace_bytes(nf)) {
        set_error("mesh_distance: workspace too small (need ls_mesh_distance_workspace_bytes(%d))", nf);
        return LS_ERR_WORKSPACE;
    }
    const BinWs w = bin_layout(workspace, 0, 1, nf, DIST_CELLS, sizeof(Cells3));
    return distance_launch(OneMesh{vertices, nv, faces, nf, n, 0}, 1, nf, points, n, max_dist, DIST_CELLS, w, dist_out, entries, cap_entries,
                           count_out, st);
}

size_t ls_mesh_sample_workspace_bytes(int nf) {
    if (nf < 0) return 0;
    return sample_layout(nullptr, 0, nf, scan_blocks(nf)).bytes;
}

int ls_mesh_sample_f64(const double* vertices, int nv, const int32_t* faces, int nf, long long count, unsigned long long seed,
                       double* points_out, int64_t* face_out, void* workspace, size_t workspace_bytes, void* stream) {
    LS_REQUIRE(nf > 0 && nv > 0, "mesh_sample: empty mesh (nv %d, nf %d)", nv, nf);
    LS_REQUIRE((long long)nf <= SCAN_MAX_N, "mesh_sample: too many faces (%d > %lld)", nf, SCAN_MAX_N);
    LS_REQUIRE(count > 0, "mesh_sample: count must be positive, got %lld", count);
    LS_REQUIRE(vertices && faces && points_out, "mesh_sample: null vertices / faces / points_out");
    if (!workspace || workspace_bytes < ls_mesh_sample_workspace_bytes(nf)) {
        set_error("mesh_sample: workspace too small (need ls_mesh_sample_workspace_bytes(%d))", nf);
        return LS_ERR_WORKSPACE;
    }
    const int nblk = (int)scan_blocks(nf);
    const SampleWs w = sample_layout(workspace, 0, nf, nblk);
    return sample_launch(OneMesh{vertices, nv, faces, nf, count, sample_key(seed)}, 1, nf, nblk, count, w, points_out, face_out,
                         (hipStream_t)stream);
}

// ---- ragged batches: every mesh's result is bit-identical to the single-mesh op on that mesh alone
size_t ls_mesh_contains_batch_workspace_bytes(int M, long long nf_total, int hash_resolution) {
    if (M < 0 || nf_total < 0 || nf_total > INT_MAX || hash_resolution < 2 || hash_resolution > MAX_HASH_RES) return 0;
    return bin_layout(nullptr, n_offs(M), M, nf_total, (long long)M * hash_resolution * hash_resolution, sizeof(Cells2)).bytes;
}

int ls_mesh_contains_batch_f64(int M, const double* vertices, long long nv_total, const long long* vert_off, const int32_t* faces, long long nf_total,
                               const long long* face_off, const double* points, long long n_total, const long long* pt_off, int hash_resolution,
                               uint8_t* inside_out, int32_t* entries, long long cap_entries, long long* count_out, void* workspace,
                               size_t workspace_bytes, void* stream) {
    const char* op = "mesh_contains_batch";
    LS_REQUIRE(hash_resolution >= 2 && hash_resolution <= MAX_HASH_RES, "%s: hash_resolution must be in [2, %d], got %d", op, MAX_HASH_RES,
               hash_resolution);
    int rc = check_meshes(op, M, vertices, nv_total, vert_off, faces, nf_total, face_off);
    if (rc != LS_OK) return rc;
    LS_REQUIRE(n_total >= 0, "%s: negative n_total %lld", op, n_total);
    rc = check_ranges(op, "pt_off", M, pt_off, n_total, LLONG_MAX);
    if (rc != LS_OK) return rc;
    LS_REQUIRE(count_out, "%s: null count_out", op);
    LS_REQUIRE(cap_entries >= 0, "%s: negative cap_entries", op);
    LS_REQUIRE(!entries || n_total == 0 || (points && inside_out), "%s: null points / inside_out with n_total = %lld", op, n_total);
    hipStream_t st = (hipStream_t)stream;
    if (nf_total == 0) {   // every mesh is empty: nothing is inside
        LS_HIP_CHECK(hipMemsetAsync(count_out, 0, sizeof(long long), st));
        if (entries && n_total > 0) LS_HIP_CHECK(hipMemsetAsync(inside_out, 0, (size_t)n_total, st));
        return LS_OK;
    }
    const int R = hash_resolution;
    if (!workspace || workspace_bytes < ls_mesh_contains_batch_workspace_bytes(M, nf_total, R)) {
        set_error("%s: workspace too small (need ls_mesh_contains_batch_workspace_bytes(%d, %lld, %d))", op, M, nf_total, R);
        return LS_ERR_WORKSPACE;
    }
    const BinWs w = bin_layout(workspace, n_offs(M), M, nf_total, (long long)M * R * R, sizeof(Cells2));
    rc = upload_offsets(w.offs, pack_offsets(M, vert_off, face_off, pt_off, nullptr, nullptr), st);
    if (rc != LS_OK) return rc;
    return contains_launch(RaggedMeshes{vertices, faces, w.offs, M, nf_total, n_total, nullptr}, M, nf_total, points, n_total, R, w, inside_out,
                           entries, cap_entries, count_out, st);
}

size_t ls_mesh_distance_batch_workspace_bytes(int M, long long nf_total) {
    if (M < 0 || nf_total < 0 || nf_total > INT_MAX) return 0;
    return bin_layout(nullptr, n_offs(M), M, nf_total, 8 * nf_total + M, sizeof(Cells3)).bytes;
}

int ls_mesh_distance_batch_f64(int M, const double* vertices, long long nv_total, const long long* vert_off, const int32_t* faces, long long nf_total,
                               const long long* face_off, const double* points, long long n_total, const long long* pt_off, double max_dist,
                               double* dist_out, int32_t* entries, long long cap_entries, long long* count_out, void* workspace,
                               size_t workspace_bytes, void* stream) {
    const char* op = "mesh_distance_batch";
    LS_REQUIRE(max_dist > 0 && max_dist < (double)INFINITY, "%s: max_dist must be positive and finite, got %g", op, max_dist);
    int rc = check_meshes(op, M, vertices, nv_total, vert_off, faces, nf_total, face_off);
    if (rc != LS_OK) return rc;
    LS_REQUIRE(n_total >= 0, "%s: negative n_total %lld", op, n_total);
    rc = check_ranges(op, "pt_off", M, pt_off, n_total, LLONG_MAX);
    if (rc != LS_OK) return rc;
    LS_REQUIRE(count_out, "%s: null count_out", op);
    LS_REQUIRE(cap_entries >= 0, "%s: negative cap_entries", op);
    LS_REQUIRE(!entries || n_total == 0 || (points && dist_out), "%s: null points / dist_out with n_total = %lld", op, n_total);
    hipStream_t st = (hipStream_t)stream;
    if (nf_total == 0) {   // every mesh is empty: infinitely far away
        LS_HIP_CHECK(hipMemsetAsync(count_out, 0, sizeof(long long), st));
        if (entries && n_total > 0) hipLaunchKernelGGL(fill_f64_kernel, dim3(cdiv(n_total, 256)), dim3(256), 0, st, dist_out, n_total, (double)INFINITY);
        LS_LAUNCH_CHECK();
        return LS_OK;
    }
    if (!workspace || workspace_bytes < ls_mesh_distance_batch_workspace_bytes(M, nf_total)) {
        set_error("%s: workspace too small (need ls_mesh_distance_batch_workspace_bytes(%d, %lld))", op, M, nf_total);
        return LS_ERR_WORKSPACE;
    }
    std::vector<long long> cell_off(M + 1, 0), axis(M + 1, 0);
    for (int m = 0; m < M; ++m) {
        axis[m] = dist_axis_cap(face_off[m + 1] - face_off[m]);
        cell_off[m + 1] = cell_off[m] + axis[m] * axis[m] * axis[m];
    }
    const long long cells = cell_off[M];   // <= 8 nf_total + M
    const BinWs w = bin_layout(workspace, n_offs(M), M, nf_total, cells, sizeof(Cells3));
    rc = upload_offsets(w.offs, pack_offsets(M, vert_off, face_off, pt_off, cell_off.data(), axis.data()), st);
    if (rc != LS_OK) return rc;
    return distance_launch(RaggedMeshes{vertices, faces, w.offs, M, nf_total, n_total, nullptr}, M, nf_total, points, n_total, max_dist, cells, w,
                           dist_out, entries, cap_entries, count_out, st);
}

size_t ls_mesh_sample_batch_workspace_bytes(int M, long long nf_total) {
    if (M < 0 || nf_total < 0 || nf_total > INT_MAX) return 0;
    return sample_layout(nullptr, n_offs(M), nf_total, scan_blocks(nf_total) + M).bytes;   // at least the sum over meshes of scan_blocks(nf_m)
}

int ls_mesh_sample_batch_f64(int M, const double* vertices, long long nv_total, const long long* vert_off, const int32_t* faces, long long nf_total,
                             const long long* face_off, long long count_total, const long long* count_off, const unsigned long long* seeds,
                             double* points_out, int64_t* face_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* op = "mesh_sample_batch";
    int rc = check_meshes(op, M, vertices, nv_total, vert_off, faces, nf_total, face_off);
    if (rc != LS_OK) return rc;
    LS_REQUIRE(count_total >= 0, "%s: negative count_total %lld", op, count_total);
    rc = check_ranges(op, "count_off", M, count_off, count_total, LLONG_MAX);
    if (rc != LS_OK) return rc;
    std::vector<long long> blk_off(M + 1, 0);
    for (int m = 0; m < M; ++m) {
        const long long nf = face_off[m + 1] - face_off[m], nv = vert_off[m + 1] - vert_off[m], count = count_off[m + 1] - count_off[m];
        LS_REQUIRE(count == 0 || (nf > 0 && nv > 0), "%s: mesh %d: empty mesh (nv %lld, nf %lld) cannot give %lld samples", op, m, nv, nf, count);
        LS_REQUIRE(nf <= SCAN_MAX_N, "%s: mesh %d: too many faces (%lld > %lld)", op, m, nf, SCAN_MAX_N);
        blk_off[m + 1] = blk_off[m] + (count > 0 ? scan_blocks(nf) : 0);   // only the sampled meshes are scanned
    }
    if (count_total == 0) return LS_OK;
    LS_REQUIRE(points_out && seeds, "%s: null points_out / seeds", op);
    if (!workspace || workspace_bytes < ls_mesh_sample_batch_workspace_bytes(M, nf_total)) {
        set_error("%s: workspace too small (need ls_mesh_sample_batch_workspace_bytes(%d, %lld))", op, M, nf_total);
        return LS_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const SampleWs w = sample_layout(workspace, n_offs(M), nf_total, scan_blocks(nf_total) + M);
    rc = upload_offsets(w.offs, pack_offsets(M, vert_off, face_off, count_off, blk_off.data(), nullptr), st);
    if (rc != LS_OK) return rc;
    return sample_launch(RaggedMeshes{vertices, faces, w.offs, M, nf_total, count_total, seeds}, M, nf_total, (int)blk_off[M], count_total, w,
                         points_out, face_out, st);
}

}  // extern "C"

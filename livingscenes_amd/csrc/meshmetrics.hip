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
#include "ls_common.h"

// bit-identity with numpy's float64 arithmetic: no contraction of a * b + c into an fma anywhere in this file
#pragma clang fp contract(off)

namespace ls {
namespace mm {

constexpr int SCAN_T = 256, SCAN_ITEMS = 16, SCAN_PER_BLOCK = SCAN_T * SCAN_ITEMS;
constexpr int SCAN_MAX_BLOCKS = 4096;                 // the top-level scan: 1024 threads x 4
constexpr long long SCAN_MAX_N = (long long)SCAN_PER_BLOCK * SCAN_MAX_BLOCKS;
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

__host__ __device__ inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline long long scan_blocks(long long n) { return (n + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK; }

// ------------------------------------------------------------------------------------------------ block-wise scan (count -> offsets, area -> cumsum)
template <typename T>
__device__ T block_scan_excl(T v, T* lds, T& total) {    // SCAN_T threads; exclusive prefix of v in thread order
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (int o = 1; o < SCAN_T; o <<= 1) {
        const T a = tid >= o ? lds[tid - o] : T(0);
        __syncthreads();
        lds[tid] += a;
        __syncthreads();
    }
    total = lds[SCAN_T - 1];
    const T ex = tid > 0 ? lds[tid - 1] : T(0);
    __syncthreads();
    return ex;
}

template <typename In, typename T>
__global__ __launch_bounds__(SCAN_T) void scan_reduce_kernel(const In* __restrict__ x, long long n, T* __restrict__ blk) {
    __shared__ T lds[SCAN_T];
    const long long base = (long long)blockIdx.x * SCAN_PER_BLOCK + (long long)threadIdx.x * SCAN_ITEMS;
    T s = T(0);
    for (int k = 0; k < SCAN_ITEMS; ++k)
        if (base + k < n) s += (T)x[base + k];
    T total;
    block_scan_excl<T>(s, lds, total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// exclusive scan of the nblk block sums in place; total_out (nullable) = sum of everything
template <typename T>
__global__ __launch_bounds__(1024) void scan_top_kernel(T* __restrict__ blk, int nblk, long long* __restrict__ total_out) {
    __shared__ T lds[1024];
    const int tid = threadIdx.x;
    const int per = (nblk + 1023) / 1024;
    const int b0 = tid * per;
    T s = T(0);
    for (int k = 0; k < per; ++k)
        if (b0 + k < nblk) s += blk[b0 + k];
    lds[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const T a = tid >= o ? lds[tid - o] : T(0);
        __syncthreads();
        lds[tid] += a;
        __syncthreads();
    }
    T run = tid > 0 ? lds[tid - 1] : T(0);
    for (int k = 0; k < per; ++k)
        if (b0 + k < nblk) {
            const T v = blk[b0 + k];
            blk[b0 + k] = run;
            run += v;
        }
    if (tid == 1023 && total_out) *total_out = (long long)lds[1023];
}

// out[i] = prefix of x: exclusive (INCL = false) or inclusive, the offsets of the block sums added
template <typename In, typename T, bool INCL>
__global__ __launch_bounds__(SCAN_T) void scan_apply_kernel(const In* __restrict__ x, long long n, const T* __restrict__ blk,
                                                            T* __restrict__ out) {
    __shared__ T lds[SCAN_T];
    const long long base = (long long)blockIdx.x * SCAN_PER_BLOCK + (long long)threadIdx.x * SCAN_ITEMS;
    T v[SCAN_ITEMS];
    T s = T(0);
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        v[k] = base + k < n ? (T)x[base + k] : T(0);
        s += v[k];
    }
    T total;
    T run = block_scan_excl<T>(s, lds, total) + blk[blockIdx.x];
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (INCL) run += v[k];
        if (base + k < n) out[base + k] = run;
        if (!INCL) run += v[k];
    }
}

template <typename In, typename T, bool INCL>
static void scan(const In* x, long long n, T* blk, T* out, long long* total_out, hipStream_t st) {
    const int nblk = (int)scan_blocks(n);
    hipLaunchKernelGGL((scan_reduce_kernel<In, T>), dim3(nblk), dim3(SCAN_T), 0, st, x, n, blk);
    hipLaunchKernelGGL((scan_top_kernel<T>), dim3(1), dim3(1024), 0, st, blk, nblk, total_out);
    hipLaunchKernelGGL((scan_apply_kernel<In, T, INCL>), dim3(nblk), dim3(SCAN_T), 0, st, x, n, blk, out);
}

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
// (scale = (R-1)/(max-min), translate = 0.5 - scale*min) and, for max_dist > 0, the distance grid.  One workgroup.
__global__ __launch_bounds__(1024) void bbox_kernel(const double* __restrict__ V, int nv, const int32_t* __restrict__ F, int nf, int R,
                                                    double max_dist, Params* __restrict__ prm) {
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
            const int g = cells >= (double)DIST_GRID_AXIS ? DIST_GRID_AXIS : (cells >= 1.0 ? (int)cells : 1);
            prm->org[a] = org;
            prm->top[a] = top;
            prm->g[a] = g;
            prm->h[a] = (top - org) / (double)g;
        }
    }
    prm->valid = sbad[0] & 1 ? -1 : valid;
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

__global__ __launch_bounds__(256) void contains_prep_kernel(const double* __restrict__ V, int nv, const int32_t* __restrict__ F, int nf, int R,
                                                            const Params* __restrict__ prm, double* __restrict__ tri, Cells2* __restrict__ tcell,
                                                            int* __restrict__ cell_count) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nf || prm->valid != 1) return;
    const Params p = *prm;
    double t[3][3];
    for (int c = 0; c < 3; ++c) {
        double v[3];
        corner(V, nv, F, f, c, v);   // valid == 1: every index is in range
        for (int a = 0; a < 3; ++a) {
            t[c][a] = rescale(p, a, v[a]);
            tri[(size_t)f * 9 + c * 3 + a] = t[c][a];
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
    tcell[f] = cl;
    for (int x = cl.x0; x <= cl.x1; ++x)
        for (int y = cl.y0; y <= cl.y1; ++y) atomicAdd(&cell_count[(size_t)x * R + y], 1);
}

// entries of cell c: entries[start[c] .. start[c] + count[c]); cursor (zeroed) counts the slots taken.  Nothing is written at or past cap.
__global__ __launch_bounds__(256) void contains_fill_kernel(int nf, int R, const Params* __restrict__ prm, const Cells2* __restrict__ tcell,
                                                            const long long* __restrict__ start, int* __restrict__ cursor,
                                                            int32_t* __restrict__ entries, long long cap) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nf || prm->valid != 1) return;
    const Cells2 cl = tcell[f];
    for (int x = cl.x0; x <= cl.x1; ++x)
        for (int y = cl.y0; y <= cl.y1; ++y) {
            const size_t c = (size_t)x * R + y;
            const long long o = start[c] + atomicAdd(&cursor[c], 1);
            if (o < cap) entries[o] = f;
        }
}

// one point against the triangles of its hash cell: parity of the strict 2-D hits above and below it (inside_mesh.py:39-154)
__global__ __launch_bounds__(256) void contains_query_kernel(const double* __restrict__ P, long long n, int R, const Params* __restrict__ prm,
                                                             const double* __restrict__ tri, const long long* __restrict__ start,
                                                             const int* __restrict__ count, const int32_t* __restrict__ entries,
                                                             const long long* __restrict__ total, long long cap, uint8_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Params p = *prm;
    bool inside = false;
    if (p.valid == 1 && *total <= cap) {
        const double px = rescale(p, 0, P[i * 3 + 0]), py = rescale(p, 1, P[i * 3 + 1]), pz = rescale(p, 2, P[i * 3 + 2]);
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
    out[i] = inside ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ distance under a cap
struct Cells3 { int lo[3], hi[3]; };

__device__ __forceinline__ int grid_cell(const Params& p, int a, double v) {
    const double t = floor((v - p.org[a]) / p.h[a]);
    const int i = (int)fmin(fmax(t, -1.0), (double)p.g[a]);
    return min(max(i, 0), p.g[a] - 1);
}

__global__ __launch_bounds__(256) void dist_prep_kernel(const double* __restrict__ V, int nv, const int32_t* __restrict__ F, int nf, double max_dist,
                                                        const Params* __restrict__ prm, double* __restrict__ tri, Cells3* __restrict__ tcell,
                                                        int* __restrict__ cell_count) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nf || prm->valid < 0) return;
    const Params p = *prm;
    double t[3][3];
    for (int c = 0; c < 3; ++c) {
        corner(V, nv, F, f, c, t[c]);
        for (int a = 0; a < 3; ++a) tri[(size_t)f * 9 + c * 3 + a] = t[c][a];
    }
    Cells3 cl;
    for (int a = 0; a < 3; ++a) {
        const double mn = fmin(fmin(t[0][a], t[1][a]), t[2][a]), mx = fmax(fmax(t[0][a], t[1][a]), t[2][a]);
        cl.lo[a] = grid_cell(p, a, mn - max_dist);
        cl.hi[a] = grid_cell(p, a, mx + max_dist);
    }
    tcell[f] = cl;
    for (int x = cl.lo[0]; x <= cl.hi[0]; ++x)
        for (int y = cl.lo[1]; y <= cl.hi[1]; ++y)
            for (int z = cl.lo[2]; z <= cl.hi[2]; ++z) atomicAdd(&cell_count[((size_t)x * p.g[1] + y) * p.g[2] + z], 1);
}

__global__ __launch_bounds__(256) void dist_fill_kernel(int nf, const Params* __restrict__ prm, const Cells3* __restrict__ tcell,
                                                        const long long* __restrict__ start, int* __restrict__ cursor, int32_t* __restrict__ entries,
                                                        long long cap) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nf || prm->valid < 0) return;
    const int gy = prm->g[1], gz = prm->g[2];
    const Cells3 cl = tcell[f];
    for (int x = cl.lo[0]; x <= cl.hi[0]; ++x)
        for (int y = cl.lo[1]; y <= cl.hi[1]; ++y)
            for (int z = cl.lo[2]; z <= cl.hi[2]; ++z) {
                const size_t c = ((size_t)x * gy + y) * gz + z;
                const long long o = start[c] + atomicAdd(&cursor[c], 1);
                if (o < cap) entries[o] = f;
            }
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

__global__ __launch_bounds__(256) void dist_query_kernel(const double* __restrict__ P, long long n, double max_dist, const Params* __restrict__ prm,
                                                         const double* __restrict__ tri, const long long* __restrict__ start,
                                                         const int* __restrict__ count, const int32_t* __restrict__ entries,
                                                         const long long* __restrict__ total, long long cap, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Params p = *prm;
    double best = INFINITY;
    const double q[3] = {P[i * 3 + 0], P[i * 3 + 1], P[i * 3 + 2]};
    // outside [min - max_dist, max + max_dist] on an axis: farther than max_dist from every triangle
    const bool in_dom = q[0] >= p.org[0] && q[0] <= p.top[0] && q[1] >= p.org[1] && q[1] <= p.top[1] && q[2] >= p.org[2] && q[2] <= p.top[2];
    if (p.valid >= 0 && *total <= cap && in_dom) {
        const size_t c = ((size_t)grid_cell(p, 0, q[0]) * p.g[1] + grid_cell(p, 1, q[1])) * p.g[2] + grid_cell(p, 2, q[2]);
        const long long s = start[c];
        const int m = count[c];
        for (int k = 0; k < m; ++k) {
            const double* t = tri + (size_t)entries[s + k] * 9;
            best = fmin(best, point_triangle_d2(q, t, t + 3, t + 6));
        }
    }
    const double d = sqrt(best);
    out[i] = d < max_dist ? d : INFINITY;
}

__global__ __launch_bounds__(256) void fill_f64_kernel(double* __restrict__ out, long long n, double v) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = v;
}

// ------------------------------------------------------------------------------------------------ surface sampling (trimesh.sample.sample_surface)
__host__ __device__ inline unsigned long long splitmix_mix(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// uniform in [0, 1): the top 53 bits of splitmix64's output for counter j of stream `seed`
__device__ __forceinline__ double uniform(unsigned long long key, unsigned long long j) {
    return (double)(splitmix_mix(key + (j + 1ull) * 0x9E3779B97F4A7C15ull) >> 11) * 0x1.0p-53;
}

// trimesh Trimesh.area_faces: |cross(v1 - v0, v2 - v0)| / 2, components written as np.cross does
__global__ __launch_bounds__(256) void area_kernel(const double* __restrict__ V, int nv, const int32_t* __restrict__ F, int nf,
                                                   double* __restrict__ area) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    double a[3], b[3], c[3];
    if (!corner(V, nv, F, f, 0, a) || !corner(V, nv, F, f, 1, b) || !corner(V, nv, F, f, 2, c)) { area[f] = 0.0; return; }
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const double wx = c[0] - a[0], wy = c[1] - a[1], wz = c[2] - a[2];
    const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
    area[f] = sqrt(cx * cx + cy * cy + cz * cz) / 2.0;
}

__global__ __launch_bounds__(256) void sample_kernel(const double* __restrict__ V, int nv, const int32_t* __restrict__ F, int nf,
                                                     const double* __restrict__ cum, long long count, unsigned long long key,
                                                     double* __restrict__ pts, int64_t* __restrict__ face_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
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
        pts[i * 3 + k] = ok ? (r1 * (b[k] - a[k]) + r2 * (c[k] - a[k])) + a[k] : NAN;
    if (face_out) face_out[i] = lo;
}

}  // namespace mm
}  // namespace ls

using namespace ls;
using namespace ls::mm;

namespace {
struct Layout {   // carve a workspace in 256-byte aligned pieces
    size_t off = 0;
    template <typename T>
    T* take(char* base, size_t n) {
        T* p = base ? (T*)(base + off) : nullptr;
        off = align256(off + n * sizeof(T));
        return p;
    }
};
struct BinWs {
    Params* prm;
    double* tri;
    void* tcell;
    int* cell_count;
    long long* start;
    long long* blk;
};
BinWs bin_layout(char* ws, int nf, long long cells, size_t cell_rec, size_t* bytes) {
    Layout L;
    BinWs w;
    w.prm = L.take<Params>(ws, 1);
    w.tri = L.take<double>(ws, (size_t)nf * 9);
    w.tcell = L.take<char>(ws, (size_t)nf * cell_rec);
    w.cell_count = L.take<int>(ws, (size_t)cells);
    w.start = L.take<long long>(ws, (size_t)cells);
    w.blk = L.take<long long>(ws, (size_t)scan_blocks(cells));
    if (bytes) *bytes = L.off;
    return w;
}
}  // namespace

extern "C" {

size_t ls_mesh_contains_workspace_bytes(int nf, int hash_resolution) {
    if (nf < 0 || hash_resolution < 2 || hash_resolution > MAX_HASH_RES) return 0;
    size_t b;
    bin_layout(nullptr, nf, (long long)hash_resolution * hash_resolution, sizeof(Cells2), &b);
    return b;
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
    const long long cells = (long long)R * R;
    if (!workspace || workspace_bytes < ls_mesh_contains_workspace_bytes(nf, R)) {
        set_error("mesh_contains: workspace too small (need ls_mesh_contains_workspace_bytes(%d, %d))", nf, R);
        return LS_ERR_WORKSPACE;
    }
    BinWs w = bin_layout((char*)workspace, nf, cells, sizeof(Cells2), nullptr);
    Cells2* tcell = (Cells2*)w.tcell;
    const int fb = (int)cdiv(nf, 256);
    LS_HIP_CHECK(hipMemsetAsync(w.cell_count, 0, (size_t)cells * sizeof(int), st));
    hipLaunchKernelGGL(bbox_kernel, dim3(1), dim3(1024), 0, st, vertices, nv, faces, nf, R, 0.0, w.prm);
    hipLaunchKernelGGL(contains_prep_kernel, dim3(fb), dim3(256), 0, st, vertices, nv, faces, nf, R, w.prm, w.tri, tcell, w.cell_count);
    scan<int, long long, false>(w.cell_count, cells, w.blk, w.start, count_out, st);
    LS_LAUNCH_CHECK();
    if (!entries) return LS_OK;   // sizing call
    // the fill takes its slots with a zeroed cursor in cell_count, which ends equal to the counts the query reads
    LS_HIP_CHECK(hipMemsetAsync(w.cell_count, 0, (size_t)cells * sizeof(int), st));
    hipLaunchKernelGGL(contains_fill_kernel, dim3(fb), dim3(256), 0, st, nf, R, w.prm, tcell, w.start, w.cell_count, entries, cap_entries);
    if (n > 0)
        hipLaunchKernelGGL(contains_query_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, points, n, R, w.prm, w.tri, w.start, w.cell_count,
                           entries, count_out, cap_entries, inside_out);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

size_t ls_mesh_distance_workspace_bytes(int nf) {
    if (nf < 0) return 0;
    size_t b;
    bin_layout(nullptr, nf, DIST_CELLS, sizeof(Cells3), &b);
    return b;
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
    BinWs w = bin_layout((char*)workspace, nf, DIST_CELLS, sizeof(Cells3), nullptr);
    Cells3* tcell = (Cells3*)w.tcell;
    const int fb = (int)cdiv(nf, 256);
    LS_HIP_CHECK(hipMemsetAsync(w.cell_count, 0, (size_t)DIST_CELLS * sizeof(int), st));
    hipLaunchKernelGGL(bbox_kernel, dim3(1), dim3(1024), 0, st, vertices, nv, faces, nf, 2, max_dist, w.prm);
    hipLaunchKernelGGL(dist_prep_kernel, dim3(fb), dim3(256), 0, st, vertices, nv, faces, nf, max_dist, w.prm, w.tri, tcell, w.cell_count);
    scan<int, long long, false>(w.cell_count, DIST_CELLS, w.blk, w.start, count_out, st);
    LS_LAUNCH_CHECK();
    if (!entries) return LS_OK;
    LS_HIP_CHECK(hipMemsetAsync(w.cell_count, 0, (size_t)DIST_CELLS * sizeof(int), st));
    hipLaunchKernelGGL(dist_fill_kernel, dim3(fb), dim3(256), 0, st, nf, w.prm, tcell, w.start, w.cell_count, entries, cap_entries);
    if (n > 0)
        hipLaunchKernelGGL(dist_query_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, points, n, max_dist, w.prm, w.tri, w.start, w.cell_count,
                           entries, count_out, cap_entries, dist_out);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

size_t ls_mesh_sample_workspace_bytes(int nf) {
    if (nf < 0) return 0;
    Layout L;
    L.take<double>(nullptr, (size_t)nf);
    L.take<double>(nullptr, (size_t)nf);
    L.take<double>(nullptr, (size_t)scan_blocks(nf));
    return L.off;
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
    hipStream_t st = (hipStream_t)stream;
    Layout L;
    char* ws = (char*)workspace;
    double* area = L.take<double>(ws, (size_t)nf);
    double* cum = L.take<double>(ws, (size_t)nf);
    double* blk = L.take<double>(ws, (size_t)scan_blocks(nf));
    hipLaunchKernelGGL(area_kernel, dim3(cdiv(nf, 256)), dim3(256), 0, st, vertices, nv, faces, nf, area);
    scan<double, double, true>(area, nf, blk, cum, nullptr, st);
    hipLaunchKernelGGL(sample_kernel, dim3(cdiv(count, 256)), dim3(256), 0, st, vertices, nv, faces, nf, cum, count,
                       splitmix_mix(seed + 0x9E3779B97F4A7C15ull), points_out, face_out);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

}  // extern "C"

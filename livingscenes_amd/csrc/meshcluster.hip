// meshcluster.hip -- decimation on the device: vertex clustering on a uniform grid with quadric-optimal representatives (Lindstrom, "Out-of-
// core simplification of large polygonal models", 2000, with a regularised solve).  The definition is in include/livingscenes_hip.h
// (ls_mesh_cluster_f64) and, as NumPy, in tests/cluster_oracle.py; this file follows it to the letter:
//   grid        lo = per-axis minimum over all vertices, ext = largest axis extent (1 when 0), h = ext / r, key = (c_x r + c_y) r + c_z
//   resolution  bisection of r in [1, r_max] on n_keep(r) = faces with three different keys; a probe is one pass over the faces, and every
//               thread of probe k replays the bisection from the counts of probes 0 .. k-1, so a probe is one launch and nothing else
//   faces       a hash keyed by the sorted key triple holds a count and the lowest face index per triple: odd groups keep that face
//   cells       a bitmap of r^3 bits per mesh and a popcount scan give every output cell its rank in ascending key order
//   vertices    per output cell one list of its input vertices and its face corners (count, scan, fill), sorted by the cell's thread and
//               summed in ascending order -- no floating-point atomics, so a mesh's bits are the same alone, in any batch and in any run
// Every kernel is written once, for a mesh locator (OneMesh / RaggedMeshes, as meshmetrics.hip); the number of launches does not depend
// on M.  Integer atomics count, set bitmap bits, claim hash slots and list slots; the hash probe loop is bounded by the table size.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "ls_common.h"
#include "ls_ragged.h"
#include "ls_scan.h"

// the arithmetic of the definition as written: no contraction of a * b + c into an fma anywhere in this file
#pragma clang fp contract(off)

namespace ls {
namespace mcl {

constexpr int R_MAX = 256;          // cells per axis at most: keys below 2^24
constexpr int MAX_PROBES = 8;       // bisection steps for r_max = 256
static_assert((1 << MAX_PROBES) >= R_MAX, "a bisection of [1, R_MAX] takes at most MAX_PROBES probes");
constexpr double REG = 1e-3;        // (A + REG tr(A) I) delta = g

enum { FACE_OVERFLOW = -1, FACE_FLAT = -2, FACE_BAD = -3 };   // face state below 0; >= 0: the face's hash slot

// per-mesh state the device derives (first bytes of the workspace)
struct Params {
    double lo[3], ext, h;
    int r;                  // 0: nf <= f_target, the mesh is copied
    int status;             // LS_OK, LS_ERR_INVALID (a face index out of range), LS_ERR_WORKSPACE (hash overflow)
    int nv_out;
    int cnt[MAX_PROBES];    // n_keep of the probes
};

// ------------------------------------------------------------------------------------------------ which mesh: one, or one of a ragged batch
struct MeshRef {
    const double* V;
    long long nv;
    const long long* F;
    long long nf;
    long long v0, f0;      // global index of the mesh's first vertex / face
    long long t0, T;       // its hash table: first slot, slots
};

struct OneMesh {
    const double* V;
    long long nv;
    const long long* F;
    long long nf, T;
    __device__ long long verts() const { return nv; }
    __device__ long long faces() const { return nf; }
    __device__ int vert_owner(long long) const { return 0; }
    __device__ int face_owner(long long) const { return 0; }
    __device__ MeshRef mesh(int) const { return {V, nv, F, nf, 0, 0, 0, T}; }
};

enum { OFF_V = 0, OFF_F, OFF_T, OFF_ARRAYS };   // the device copy of a batch's offsets: vertices, faces, hash slots

struct RaggedMeshes {
    const double* V;
    const long long* F;
    const long long* offs;
    int M;
    long long nv_total, nf_total;
    __device__ const long long* off(int k) const { return offs + (size_t)k * (M + 1); }
    __device__ long long verts() const { return nv_total; }
    __device__ long long faces() const { return nf_total; }
    __device__ int vert_owner(long long i) const { return owner(off(OFF_V), M, i); }
    __device__ int face_owner(long long g) const { return owner(off(OFF_F), M, g); }
    __device__ MeshRef mesh(int m) const {
        const long long *vo = off(OFF_V), *fo = off(OFF_F), *to = off(OFF_T);
        return {V + vo[m] * 3, vo[m + 1] - vo[m], F + fo[m] * 3, fo[m + 1] - fo[m], vo[m], fo[m], to[m], to[m + 1] - to[m]};
    }
};

// ------------------------------------------------------------------------------------------------ grid
// key of v at resolution r; the clamp to [0, r - 1] before the cast keeps any value (NaN included) inside the grid
__device__ __forceinline__ void cell_of(const double* __restrict__ v, const double* lo, double h, int r, int (&c)[3]) {
    for (int a = 0; a < 3; ++a) c[a] = (int)fmin(fmax(floor((v[a] - lo[a]) / h), 0.0), (double)(r - 1));
}
__device__ __forceinline__ int key_of(const double* __restrict__ v, const double* lo, double h, int r) {
    int c[3];
    cell_of(v, lo, h, r, c);
    return (c[0] * r + c[1]) * r + c[2];
}

// the keys of face f's corners; false (nothing read through the bad index) when a corner names no vertex
__device__ __forceinline__ bool face_keys(const MeshRef& M, long long f, const double* lo, double h, int r, int (&k)[3]) {
    for (int c = 0; c < 3; ++c) {
        const long long vi = M.F[f * 3 + c];
        if ((unsigned long long)vi >= (unsigned long long)M.nv) return false;
        k[c] = key_of(M.V + vi * 3, lo, h, r);
    }
    return true;
}

// one workgroup per mesh: lo, ext; cnt zeroed
template <class Meshes>
__global__ __launch_bounds__(1024) void setup_kernel(Meshes L, Params* __restrict__ prm) {
    __shared__ double slo[3][1024], shi[3][1024];
    const int m = blockIdx.x, tid = threadIdx.x;
    const MeshRef M = L.mesh(m);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long i = tid; i < M.nv; i += 1024)
        for (int a = 0; a < 3; ++a) {
            lo[a] = fmin(lo[a], M.V[i * 3 + a]);
            hi[a] = fmax(hi[a], M.V[i * 3 + a]);
        }
    for (int a = 0; a < 3; ++a) { slo[a][tid] = lo[a]; shi[a][tid] = hi[a]; }
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o)
            for (int a = 0; a < 3; ++a) {
                slo[a][tid] = fmin(slo[a][tid], slo[a][tid + o]);
                shi[a][tid] = fmax(shi[a][tid], shi[a][tid + o]);
            }
        __syncthreads();
    }
    if (tid != 0) return;
    Params& p = prm[m];
    double ext = 0;
    for (int a = 0; a < 3; ++a) {
        p.lo[a] = slo[a][0];
        ext = fmax(ext, shi[a][0] - slo[a][0]);
    }
    p.ext = ext > 0 ? ext : 1.0;   // an empty or one-point mesh (and a non-finite one, which is not supported): any grid will do
    p.h = p.ext;
    p.r = 0;
    p.status = LS_OK;
    p.nv_out = 0;
    for (int k = 0; k < MAX_PROBES; ++k) p.cnt[k] = 0;
}

// the bisection after `probes` probes: lo (== r* when lo == hi), hi
__device__ __forceinline__ void bisect_replay(const Params& p, int probes, int f_target, int r_max, int& lo, int& hi) {
    lo = 1;
    hi = r_max;
    for (int k = 0; k < probes && lo < hi; ++k) {
        const int mid = (lo + hi + 1) / 2;
        if (p.cnt[k] <= f_target) lo = mid;
        else hi = mid - 1;
    }
}

// probe k: cnt[k] of every mesh that is still searching = n_keep(mid).  A workgroup adds up the faces of its first face's mesh in LDS.
template <class Meshes>
__global__ __launch_bounds__(256) void probe_kernel(Meshes L, Params* __restrict__ prm, int k, int f_target, int r_max) {
    __shared__ int s_cnt;
    const long long g0 = (long long)blockIdx.x * 256, g = g0 + threadIdx.x;
    const int m0 = L.face_owner(g0);
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    if (g < L.faces()) {
        const int m = L.face_owner(g);
        const MeshRef M = L.mesh(m);
        if (M.nf > f_target) {
            int lo, hi;
            bisect_replay(prm[m], k, f_target, r_max, lo, hi);
            if (lo < hi) {
                const int r = (lo + hi + 1) / 2;
                int key[3];
                if (face_keys(M, g - M.f0, prm[m].lo, prm[m].ext / r, r, key) && key[0] != key[1] && key[1] != key[2] && key[0] != key[2])
                {
                    if (m == m0) atomicAdd(&s_cnt, 1);
                    else atomicAdd(&prm[m].cnt[k], 1);
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(&prm[m0].cnt[k], s_cnt);
}

template <class Meshes>
__global__ __launch_bounds__(256) void resolve_kernel(Meshes L, int M, Params* __restrict__ prm, int probes, int f_target, int r_max) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M || L.mesh(m).nf <= f_target) return;
    int lo, hi;
    bisect_replay(prm[m], probes, f_target, r_max, lo, hi);
    prm[m].r = lo;
    prm[m].h = prm[m].ext / lo;
}

// ------------------------------------------------------------------------------------------------ faces
// fkey [nf,3]: the corners' keys at r*; fstate: FACE_FLAT (two equal keys) / FACE_BAD, else unchanged
template <class Meshes>
__global__ __launch_bounds__(256) void face_key_kernel(Meshes L, Params* __restrict__ prm, int* __restrict__ fkey, int* __restrict__ fstate) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= L.faces()) return;
    const int m = L.face_owner(g);
    const Params& p = prm[m];
    if (p.r == 0) return;
    const MeshRef M = L.mesh(m);
    int k[3] = {0, 0, 0};
    int st = 0;
    if (!face_keys(M, g - M.f0, p.lo, p.h, p.r, k)) {
        st = FACE_BAD;
        prm[m].status = LS_ERR_INVALID;
    } else if (k[0] == k[1] || k[1] == k[2] || k[0] == k[2]) {
        st = FACE_FLAT;
    }
    for (int c = 0; c < 3; ++c) fkey[g * 3 + c] = k[c];
    fstate[g] = st;
}

__device__ __forceinline__ void sort3(const int* __restrict__ k, int (&s)[3]) {
    int a = k[0], b = k[1], c = k[2], t;
    if (a > b) { t = a; a = b; b = t; }
    if (b > c) { t = b; b = c; c = t; }
    if (a > b) { t = a; a = b; b = t; }
    s[0] = a; s[1] = b; s[2] = c;
}

// the hash of a mesh: slot s is claimed by the first face that writes its (global) index to rep[s]; faces with the same sorted triple
// find it by comparing against the claimant's keys (written by the kernel before), count themselves and leave the lowest index in mn[s].
// At most min(nf, f_target) triples go into 2 min(nf, f_target) + 1 slots; the walk ends after T slots whatever happens.
template <class Meshes>
__global__ __launch_bounds__(256) void face_hash_kernel(Meshes L, Params* __restrict__ prm, const int* __restrict__ fkey, int* __restrict__ fstate,
                                                        int* __restrict__ rep, int* __restrict__ cnt, int* __restrict__ mn) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= L.faces()) return;
    const int m = L.face_owner(g);
    if (prm[m].r == 0 || fstate[g] < 0) return;
    const MeshRef M = L.mesh(m);
    int s3[3];
    sort3(fkey + g * 3, s3);
    const unsigned long long hsh = mix64(mix64(((unsigned long long)s3[0] << 32) | (unsigned)s3[1]) + (unsigned long long)s3[2]);
    long long s = (long long)(hsh % (unsigned long long)M.T);
    int found = FACE_OVERFLOW;
    for (long long step = 0; step < M.T; ++step) {
        const long long slot = M.t0 + s;
        int owner_face = atomicCAS(&rep[slot], -1, (int)g);
        if (owner_face == -1) owner_face = (int)g;
        int o3[3];
        sort3(fkey + (long long)owner_face * 3, o3);
        if (o3[0] == s3[0] && o3[1] == s3[1] && o3[2] == s3[2]) {
            atomicAdd(&cnt[slot], 1);
            atomicMin(&mn[slot], (int)g);
            found = (int)s;
            break;
        }
        if (++s == M.T) s = 0;
    }
    fstate[g] = found;
    if (found < 0) prm[m].status = LS_ERR_WORKSPACE;
}

// keep[g]: the face is an output face; its corners' cells enter the mesh's bitmap
template <class Meshes>
__global__ __launch_bounds__(256) void face_select_kernel(Meshes L, const Params* __restrict__ prm, const int* __restrict__ fkey,
                                                          const int* __restrict__ fstate, const int* __restrict__ cnt, const int* __restrict__ mn,
                                                          long long words_per_mesh, unsigned* __restrict__ bitmap, int* __restrict__ keep) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= L.faces()) return;
    const int m = L.face_owner(g);
    if (prm[m].r == 0) { keep[g] = 1; return; }
    const MeshRef M = L.mesh(m);
    const int st = fstate[g];
    const bool k = st >= 0 && (cnt[M.t0 + st] & 1) && mn[M.t0 + st] == (int)g;
    keep[g] = k ? 1 : 0;
    if (!k) return;
    unsigned* bm = bitmap + (size_t)m * words_per_mesh;
    for (int c = 0; c < 3; ++c) {
        const int key = fkey[g * 3 + c];
        atomicOr(&bm[key >> 5], 1u << (key & 31));
    }
}

// ------------------------------------------------------------------------------------------------ cells: ranks from the bitmap
// words of the bitmap that can hold a set bit
__device__ __forceinline__ long long live_words(const Params& p) { return p.r == 0 ? 0 : ((long long)p.r * p.r * p.r + 31) / 32; }

// block b of mesh m's bitmap (SCAN_PER_BLOCK words): the number of set bits
__global__ __launch_bounds__(SCAN_T) void bitmap_reduce_kernel(const Params* __restrict__ prm, int blocks_per_mesh, const unsigned* __restrict__ bitmap,
                                                               int* __restrict__ blk) {
    __shared__ int lds[SCAN_T];
    const int m = blockIdx.x / blocks_per_mesh, b = blockIdx.x % blocks_per_mesh;
    const long long n = live_words(prm[m]);
    const unsigned* bm = bitmap + (size_t)m * blocks_per_mesh * SCAN_PER_BLOCK;
    const long long base = (long long)b * SCAN_PER_BLOCK + (long long)threadIdx.x * SCAN_ITEMS;
    int s = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k)
        if (base + k < n) s += __popc(bm[base + k]);
    int total;
    block_scan_excl<int>(s, lds, total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// one workgroup per mesh: its block sums scanned in place, nv_out = its output cells (a copied mesh: its vertices)
template <class Meshes>
__global__ __launch_bounds__(1024) void bitmap_top_kernel(Meshes L, Params* __restrict__ prm, int blocks_per_mesh, int* __restrict__ blk) {
    const int m = blockIdx.x;
    const int total = scan_top_block<int>(blk + (size_t)m * blocks_per_mesh, blocks_per_mesh);
    if (threadIdx.x == 0) prm[m].nv_out = prm[m].r == 0 ? (int)L.mesh(m).nv : total;
}

// one workgroup: off [2][M + 1] = the packed outputs' first vertex / first face per mesh and the totals, copied to the caller's off_out
// (or, one mesh, counts_out); r_out[m] = r, or the mesh's error: its status, LS_ERR_INVALID when it reaches past the caps of a real call
template <class Meshes>
__global__ __launch_bounds__(1024) void offsets_kernel(Meshes L, int M, const Params* __restrict__ prm, const long long* __restrict__ fpos,
                                                       const long long* __restrict__ ftotal, long long* __restrict__ off, long long* __restrict__ off_out,
                                                       long long* __restrict__ counts_out, int* __restrict__ r_out, bool real, long long cap_v,
                                                       long long cap_f) {
    for (int m = threadIdx.x; m < M; m += 1024) off[m] = prm[m].nv_out;
    __syncthreads();
    const long long vtotal = scan_top_block<long long>(off, M);
    for (int m = threadIdx.x; m <= M; m += 1024) {
        if (m == M) {
            off[M] = vtotal;
            off[2 * M + 1] = L.faces() > 0 ? *ftotal : 0;
        } else {
            const MeshRef R = L.mesh(m);
            off[M + 1 + m] = R.f0 < L.faces() ? fpos[R.f0] : (L.faces() > 0 ? *ftotal : 0);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * (M + 1); i += 1024)
        if (off_out) off_out[i] = off[i];
    if (counts_out && threadIdx.x < 2) counts_out[threadIdx.x] = off[threadIdx.x == 0 ? M : 2 * M + 1];
    if (r_out)
        for (int m = threadIdx.x; m < M; m += 1024) {
            int r = prm[m].status != LS_OK ? prm[m].status : prm[m].r;
            if (real && r >= 0 && (off[m + 1] > cap_v || off[M + 1 + m + 1] > cap_f)) r = LS_ERR_INVALID;
            r_out[m] = r;
        }
}

// rank of cell `key` among the mesh's output cells (its bit is set)
__device__ __forceinline__ int cell_rank(const unsigned* __restrict__ bm, const int* __restrict__ wprefix, int key) {
    return wprefix[key >> 5] + __popc(bm[key >> 5] & ((1u << (key & 31)) - 1u));
}

// wprefix[word] = set bits of the mesh before the word; cellkey[first output vertex + rank] = key of every set bit
__global__ __launch_bounds__(SCAN_T) void bitmap_apply_kernel(const Params* __restrict__ prm, int blocks_per_mesh, const unsigned* __restrict__ bitmap,
                                                              const int* __restrict__ blk, const long long* __restrict__ off,
                                                              int* __restrict__ wprefix, int* __restrict__ cellkey, long long cap_cells) {
    __shared__ int lds[SCAN_T];
    const int m = blockIdx.x / blocks_per_mesh, b = blockIdx.x % blocks_per_mesh;
    const long long n = live_words(prm[m]);
    if ((long long)b * SCAN_PER_BLOCK >= n) return;   // the whole workgroup
    const size_t mesh0 = (size_t)m * blocks_per_mesh * SCAN_PER_BLOCK;
    const unsigned* bm = bitmap + mesh0;
    const long long base = (long long)b * SCAN_PER_BLOCK + (long long)threadIdx.x * SCAN_ITEMS;
    unsigned w[SCAN_ITEMS];
    int s = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        w[k] = base + k < n ? bm[base + k] : 0u;
        s += __popc(w[k]);
    }
    int total;
    int run = block_scan_excl<int>(s, lds, total) + blk[blockIdx.x];
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (base + k >= n) break;
        wprefix[mesh0 + base + k] = run;
        unsigned bits = w[k];
        while (bits) {
            const int bit = __ffs(bits) - 1;
            bits &= bits - 1;
            const long long j = off[m] + run++;
            if (j < cap_cells) cellkey[j] = (int)((base + k) * 32 + bit);
        }
    }
}

// ------------------------------------------------------------------------------------------------ member lists of the output cells
// Item i < nv_total is a vertex, item nv_total + g a face.  An output cell's list holds its vertices as their local index and the face
// corners that lie in it as nv + 3 f + c: ascending order of the entries is ascending vertex index, then ascending (face, corner).
// FILL = false: count[j] += 1 per entry;  FILL = true: the entry goes to entries[start[j] + count[j]++] (count zeroed again).
template <class Meshes, bool FILL>
__global__ __launch_bounds__(256) void member_kernel(Meshes L, const Params* __restrict__ prm, const int* __restrict__ fkey, const int* __restrict__ fstate,
                                                     long long words_per_mesh, const unsigned* __restrict__ bitmap, const int* __restrict__ wprefix,
                                                     const long long* __restrict__ off, int* __restrict__ count, const long long* __restrict__ start,
                                                     int* __restrict__ entries, long long cap_cells, long long cap_entries) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.verts() + L.faces()) return;
    const bool is_vertex = i < L.verts();
    const long long g = i - L.verts();
    const int m = is_vertex ? L.vert_owner(i) : L.face_owner(g);
    const Params& p = prm[m];
    if (p.r == 0) return;
    const MeshRef M = L.mesh(m);
    const unsigned* bm = bitmap + (size_t)m * words_per_mesh;
    const int* wp = wprefix + (size_t)m * words_per_mesh;
    if (!is_vertex && fstate[g] == FACE_BAD) return;
    for (int c = 0; c < (is_vertex ? 1 : 3); ++c) {
        const int key = is_vertex ? key_of(M.V + (i - M.v0) * 3, p.lo, p.h, p.r) : fkey[g * 3 + c];
        if (!((bm[key >> 5] >> (key & 31)) & 1u)) continue;
        const long long j = off[m] + cell_rank(bm, wp, key);
        if (j >= cap_cells) continue;
        const int k = atomicAdd(&count[j], 1);
        if (FILL) {
            const long long o = start[j] + k;
            if (o < cap_entries) entries[o] = is_vertex ? (int)(i - M.v0) : (int)(M.nv + (g - M.f0) * 3 + c);
        }
    }
}

// ascending heap sort of a[0 .. n): in place, O(n log n) whatever the input
__device__ void heap_sort(int* __restrict__ a, int n) {
    auto sift = [&](int root, int end) {
        const int v = a[root];
        for (;;) {
            int child = 2 * root + 1;
            if (child >= end) break;
            if (child + 1 < end && a[child + 1] > a[child]) ++child;
            if (a[child] <= v) break;
            a[root] = a[child];
            root = child;
        }
        a[root] = v;
    };
    for (int i = n / 2 - 1; i >= 0; --i) sift(i, n);
    for (int end = n - 1; end > 0; --end) {
        const int t = a[0];
        a[0] = a[end];
        a[end] = t;
        sift(0, end);
    }
}

// (A + lam I) x = g for the symmetric positive definite A + lam I (condition <= 1 + 1 / REG): elimination without pivoting
__device__ __forceinline__ void solve3(const double (&A)[6], double lam, const double (&g)[3], double (&x)[3]) {
    const double a00 = A[0] + lam, a01 = A[1], a02 = A[2], a11 = A[3] + lam, a12 = A[4], a22 = A[5] + lam;
    const double l10 = a01 / a00, l20 = a02 / a00;
    const double b11 = a11 - l10 * a01, b12 = a12 - l10 * a02, b22 = a22 - l20 * a02;
    const double l21 = b12 / b11;
    const double c22 = b22 - l21 * b12;
    const double y0 = g[0], y1 = g[1] - l10 * y0, y2 = g[2] - l20 * y0 - l21 * y1;
    x[2] = y2 / c22;
    x[1] = (y1 - b12 * x[2]) / b11;
    x[0] = (y0 - a01 * x[1] - a02 * x[2]) / a00;
}

// one thread per output vertex: a copied mesh's vertex as it is, else the cell's representative
template <class Meshes>
__global__ __launch_bounds__(256) void vertex_kernel(Meshes L, int nmesh, const Params* __restrict__ prm, const long long* __restrict__ off,
                                                     const int* __restrict__ cellkey, const int* __restrict__ count, const long long* __restrict__ start,
                                                     int* __restrict__ entries, long long cap_entries, double* __restrict__ out, long long cap_v) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= off[nmesh] || j >= cap_v) return;
    const int m = owner(off, nmesh, j);
    const Params p = prm[m];
    const MeshRef M = L.mesh(m);
    if (p.r == 0) {
        for (int a = 0; a < 3; ++a) out[j * 3 + a] = M.V[(j - off[m]) * 3 + a];
        return;
    }
    const int n = count[j];
    if (start[j] + n > cap_entries) return;   // cannot happen: the lists hold at most nv + 3 nf entries
    int* list = entries + start[j];
    heap_sort(list, n);
    double sum[3] = {0, 0, 0};
    int k = 0;
    for (; k < n && list[k] < M.nv; ++k)
        for (int a = 0; a < 3; ++a) sum[a] = sum[a] + M.V[(long long)list[k] * 3 + a];
    double xbar[3];
    for (int a = 0; a < 3; ++a) xbar[a] = sum[a] / (double)k;   // k >= 1: an output cell is the cell of a face corner, a vertex
    double A[6] = {0, 0, 0, 0, 0, 0}, gv[3] = {0, 0, 0};
    for (; k < n; ++k) {
        const long long f = (list[k] - M.nv) / 3;
        const double* p0 = M.V + M.F[f * 3 + 0] * 3;
        const double* p1 = M.V + M.F[f * 3 + 1] * 3;
        const double* p2 = M.V + M.F[f * 3 + 2] * 3;
        const double ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
        const double wx = p2[0] - p0[0], wy = p2[1] - p0[1], wz = p2[2] - p0[2];
        const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
        const double ar = sqrt(nx * nx + ny * ny + nz * nz);
        if (ar == 0) continue;
        const double hx = nx / ar, hy = ny / ar, hz = nz / ar;
        const double d = hx * (p0[0] - xbar[0]) + hy * (p0[1] - xbar[1]) + hz * (p0[2] - xbar[2]);
        A[0] += ar * (hx * hx); A[1] += ar * (hx * hy); A[2] += ar * (hx * hz);
        A[3] += ar * (hy * hy); A[4] += ar * (hy * hz); A[5] += ar * (hz * hz);
        const double ad = ar * d;
        gv[0] += ad * hx; gv[1] += ad * hy; gv[2] += ad * hz;
    }
    const double tr = A[0] + A[3] + A[5];
    double delta[3] = {0, 0, 0};
    if (tr != 0) solve3(A, REG * tr, gv, delta);
    const int key = cellkey[j];
    const int c[3] = {key / (p.r * p.r), (key / p.r) % p.r, key % p.r};
    for (int a = 0; a < 3; ++a) {
        const double x = xbar[a] + delta[a];
        out[j * 3 + a] = fmin(fmax(x, p.lo[a] + (double)c[a] * p.h), p.lo[a] + (double)(c[a] + 1) * p.h);
    }
}

// output faces: ascending input order (fpos = the exclusive scan of keep), corner order kept, indices = the ranks of the corners' cells
template <class Meshes>
__global__ __launch_bounds__(256) void face_out_kernel(Meshes L, const Params* __restrict__ prm, const int* __restrict__ fkey, const int* __restrict__ keep,
                                                       const long long* __restrict__ fpos, long long words_per_mesh, const unsigned* __restrict__ bitmap,
                                                       const int* __restrict__ wprefix, long long* __restrict__ out, long long cap_f) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= L.faces() || !keep[g]) return;
    const long long o = fpos[g];
    if (o >= cap_f) return;
    const int m = L.face_owner(g);
    if (prm[m].r == 0) {
        const MeshRef M = L.mesh(m);
        for (int c = 0; c < 3; ++c) out[o * 3 + c] = M.F[(g - M.f0) * 3 + c];
        return;
    }
    const unsigned* bm = bitmap + (size_t)m * words_per_mesh;
    const int* wp = wprefix + (size_t)m * words_per_mesh;
    for (int c = 0; c < 3; ++c) out[o * 3 + c] = cell_rank(bm, wp, fkey[g * 3 + c]);
}

}  // namespace mcl
}  // namespace ls

using namespace ls;
using namespace ls::mcl;

namespace {
int blocks_per_mesh(int r_max) { return (int)scan_blocks(((long long)r_max * r_max * r_max + 31) / 32); }

struct Ws {
    long long* offs;      // a batch: the device copy of the offsets
    Params* prm;          // [M]
    long long* off;       // [2][M + 1] outputs' offsets
    long long *ftotal, *ltotal;   // output faces, list entries in all
    int *fkey, *fstate, *keep;
    long long* fpos;
    long long* fblk;
    int *rep, *cnt, *mn;  // hash slots
    size_t slots;
    unsigned* bitmap;
    int* wprefix;
    int* bblk;
    int* cellkey;
    int* lcount;
    long long* lstart;
    long long* lblk;
    int* entries;
    size_t zero_bytes;    // cnt .. lcount, padding included: cleared together
    size_t bytes;         // of the whole layout
};

// the layout depends on (M, nv, nf, r_max) alone: 2 nf + M hash slots cover 2 min(nf_m, f_target) + 1 per mesh for any f_target
// (ws null: a sizing pass)
Ws layout(void* ws, size_t n_offs, int M, long long nv, long long nf, int r_max) {
    Arena a(ws);
    Ws w;
    const size_t words = (size_t)M * blocks_per_mesh(r_max) * SCAN_PER_BLOCK;
    w.offs = a.take<long long>(n_offs);
    w.prm = a.take<Params>((size_t)M);
    w.off = a.take<long long>(2 * ((size_t)M + 1));
    w.ftotal = a.take<long long>(1);
    w.ltotal = a.take<long long>(1);
    w.fkey = a.take<int>((size_t)nf * 3);
    w.fstate = a.take<int>((size_t)nf);
    w.keep = a.take<int>((size_t)nf);
    w.fpos = a.take<long long>((size_t)nf);
    w.fblk = a.take<long long>((size_t)scan_blocks(nf));
    w.slots = 2 * (size_t)nf + (size_t)M;
    w.rep = a.take<int>(w.slots);
    w.mn = a.take<int>(w.slots);
    const size_t zero_begin = a.bytes();
    w.cnt = a.take<int>(w.slots);
    w.bitmap = a.take<unsigned>(words);
    w.lcount = a.take<int>((size_t)nv);
    w.zero_bytes = a.bytes() - zero_begin;
    w.wprefix = a.take<int>(words);
    w.bblk = a.take<int>((size_t)M * blocks_per_mesh(r_max));
    w.cellkey = a.take<int>((size_t)nv);
    w.lstart = a.take<long long>((size_t)nv);
    w.lblk = a.take<long long>((size_t)scan_blocks(nv));
    w.entries = a.take<int>((size_t)nv + 3 * (size_t)nf);
    w.bytes = a.bytes();
    return w;
}

// the launch sequence: M meshes located by L, nv vertices and nf faces in all, `slots` hash slots in use.  Without outputs (a sizing
// call) it stops once the offsets are written.
template <class Meshes>
int cluster_launch(const Meshes& L, int M, long long nv, long long nf, size_t slots, int f_target, int r_max, const Ws& w,
                   double* vertices_out, long long cap_v, long long* faces_out, long long cap_f, long long* off_out, long long* counts_out,
                   int* r_out, hipStream_t st) {
    const int bpm = blocks_per_mesh(r_max);
    const long long wpm = (long long)bpm * SCAN_PER_BLOCK;
    const int fb = cdiv(nf, 256);
    const bool real = vertices_out != nullptr;
    hipLaunchKernelGGL(setup_kernel<Meshes>, dim3(M), dim3(1024), 0, st, L, w.prm);
    if (nf > 0) {
        int probes = 0;
        while ((1 << probes) < r_max) ++probes;
        for (int k = 0; k < probes; ++k) hipLaunchKernelGGL(probe_kernel<Meshes>, dim3(fb), dim3(256), 0, st, L, w.prm, k, f_target, r_max);
        hipLaunchKernelGGL(resolve_kernel<Meshes>, dim3(cdiv(M, 256)), dim3(256), 0, st, L, M, w.prm, probes, f_target, r_max);
        LS_HIP_CHECK(hipMemsetAsync(w.rep, 0xFF, slots * sizeof(int), st));   // -1: free
        LS_HIP_CHECK(hipMemsetAsync(w.mn, 0x7F, slots * sizeof(int), st));    // above every face index
        LS_HIP_CHECK(hipMemsetAsync(w.cnt, 0, w.zero_bytes, st));
        hipLaunchKernelGGL(face_key_kernel<Meshes>, dim3(fb), dim3(256), 0, st, L, w.prm, w.fkey, w.fstate);
        hipLaunchKernelGGL(face_hash_kernel<Meshes>, dim3(fb), dim3(256), 0, st, L, w.prm, w.fkey, w.fstate, w.rep, w.cnt, w.mn);
        hipLaunchKernelGGL(face_select_kernel<Meshes>, dim3(fb), dim3(256), 0, st, L, w.prm, w.fkey, w.fstate, w.cnt, w.mn, wpm, w.bitmap, w.keep);
        scan<int, long long, false>(w.keep, nf, w.fblk, w.fpos, w.ftotal, st);
    }
    hipLaunchKernelGGL(bitmap_reduce_kernel, dim3(M * bpm), dim3(SCAN_T), 0, st, w.prm, bpm, w.bitmap, w.bblk);
    hipLaunchKernelGGL(bitmap_top_kernel<Meshes>, dim3(M), dim3(1024), 0, st, L, w.prm, bpm, w.bblk);
    hipLaunchKernelGGL(offsets_kernel<Meshes>, dim3(1), dim3(1024), 0, st, L, M, w.prm, w.fpos, w.ftotal, w.off, off_out, counts_out, r_out, real,
                       cap_v, cap_f);
    LS_LAUNCH_CHECK();
    if (!real) return LS_OK;
    if (nv > 0) {
        if (nf > 0) {
            const long long cap_entries = nv + 3 * nf;
            const int ib = cdiv(nv + nf, 256);
            hipLaunchKernelGGL(bitmap_apply_kernel, dim3(M * bpm), dim3(SCAN_T), 0, st, w.prm, bpm, w.bitmap, w.bblk, w.off, w.wprefix, w.cellkey, nv);
            hipLaunchKernelGGL((member_kernel<Meshes, false>), dim3(ib), dim3(256), 0, st, L, w.prm, w.fkey, w.fstate, wpm, w.bitmap, w.wprefix, w.off,
                               w.lcount, w.lstart, w.entries, nv, cap_entries);
            scan<int, long long, false>(w.lcount, nv, w.lblk, w.lstart, w.ltotal, st);
            LS_HIP_CHECK(hipMemsetAsync(w.lcount, 0, (size_t)nv * sizeof(int), st));
            hipLaunchKernelGGL((member_kernel<Meshes, true>), dim3(ib), dim3(256), 0, st, L, w.prm, w.fkey, w.fstate, wpm, w.bitmap, w.wprefix, w.off,
                               w.lcount, w.lstart, w.entries, nv, cap_entries);
        }
        hipLaunchKernelGGL(vertex_kernel<Meshes>, dim3(cdiv(nv, 256)), dim3(256), 0, st, L, M, w.prm, w.off, w.cellkey, w.lcount, w.lstart, w.entries,
                           nv + 3 * nf, vertices_out, cap_v);
    }
    if (nf > 0)
        hipLaunchKernelGGL(face_out_kernel<Meshes>, dim3(fb), dim3(256), 0, st, L, w.prm, w.fkey, w.keep, w.fpos, wpm, w.bitmap, w.wprefix, faces_out,
                           cap_f);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

long long table_slots(long long nf, int f_target) { return nf > f_target ? 2 * (long long)f_target + 1 : 0; }

// what both entries check: sizes, f_target, r_max, the outputs (both or neither), the caps
int check_common(const char* op, long long nv, long long nf, int f_target, int r_max, const double* V, const long long* F, const double* vertices_out,
                 long long cap_v, const long long* faces_out, long long cap_f) {
    LS_REQUIRE(nv >= 0 && nf >= 0, "%s: negative size (%lld vertices, %lld faces)", op, nv, nf);
    LS_REQUIRE(nv + 3 * nf <= INT_MAX, "%s: %lld vertices + 3 * %lld faces exceed %d (int member lists)", op, nv, nf, INT_MAX);
    LS_REQUIRE(f_target >= 1, "%s: f_target must be >= 1, got %d", op, f_target);
    LS_REQUIRE(r_max >= 1 && r_max <= R_MAX, "%s: r_max must be in [1, %d], got %d", op, R_MAX, r_max);
    LS_REQUIRE((nv == 0 || V) && (nf == 0 || F), "%s: null vertices / faces with %lld vertices, %lld faces", op, nv, nf);
    LS_REQUIRE((vertices_out == nullptr) == (faces_out == nullptr), "%s: vertices_out and faces_out go together (both null: a sizing call)", op);
    LS_REQUIRE(cap_v >= 0 && cap_f >= 0, "%s: negative capacity (cap_v %lld, cap_f %lld)", op, cap_v, cap_f);
    return LS_OK;
}
}  // namespace

extern "C" {

size_t ls_mesh_cluster_workspace_bytes(long long nv, long long nf, int r_max) {
    if (nv < 0 || nf < 0 || nv + 3 * nf > INT_MAX || r_max < 1 || r_max > R_MAX) return 0;
    return layout(nullptr, 0, 1, nv, nf, r_max).bytes;
}

int ls_mesh_cluster_f64(const double* vertices, long long nv, const long long* faces, long long nf, int f_target, int r_max, double* vertices_out,
                        long long cap_v, long long* faces_out, long long cap_f, long long* counts_out, int* r_out, void* workspace,
                        size_t workspace_bytes, void* stream) {
    const char* op = "mesh_cluster";
    int rc = check_common(op, nv, nf, f_target, r_max, vertices, faces, vertices_out, cap_v, faces_out, cap_f);
    if (rc != LS_OK) return rc;
    LS_REQUIRE(nf == 0 || nv > 0, "%s: %lld faces and no vertices", op, nf);
    LS_REQUIRE(counts_out, "%s: null counts_out", op);
    if (vertices_out && nf <= f_target)
        LS_REQUIRE(nv <= cap_v && nf <= cap_f, "%s: the mesh is under the target and is copied: %lld vertices, %lld faces do not fit cap_v %lld, cap_f %lld",
                   op, nv, nf, cap_v, cap_f);
    if (!workspace || workspace_bytes < ls_mesh_cluster_workspace_bytes(nv, nf, r_max)) {
        set_error("%s: workspace too small (need ls_mesh_cluster_workspace_bytes(%lld, %lld, %d))", op, nv, nf, r_max);
        return LS_ERR_WORKSPACE;
    }
    const Ws w = layout(workspace, 0, 1, nv, nf, r_max);
    const long long T = table_slots(nf, f_target);
    return cluster_launch(OneMesh{vertices, nv, faces, nf, T}, 1, nv, nf, (size_t)T, f_target, r_max, w, vertices_out, cap_v,
                          faces_out, cap_f, nullptr, counts_out, r_out, (hipStream_t)stream);
}

size_t ls_mesh_cluster_batch_workspace_bytes(int M, long long nv_total, long long nf_total, int r_max) {
    if (M < 1 || nv_total < 0 || nf_total < 0 || nv_total + 3 * nf_total > INT_MAX || r_max < 1 || r_max > R_MAX) return 0;
    return layout(nullptr, (size_t)OFF_ARRAYS * (M + 1), M, nv_total, nf_total, r_max).bytes;
}

int ls_mesh_cluster_batch_f64(int M, const double* vertices, long long nv_total, const long long* vert_off, const long long* faces, long long nf_total,
                              const long long* face_off, int f_target, int r_max, double* vertices_out, long long cap_v, long long* faces_out,
                              long long cap_f, long long* off_out, int* r_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* op = "mesh_cluster_batch";
    LS_REQUIRE(M >= 1, "%s: M must be >= 1, got %d", op, M);
    int rc = check_common(op, nv_total, nf_total, f_target, r_max, vertices, faces, vertices_out, cap_v, faces_out, cap_f);
    if (rc != LS_OK) return rc;
    rc = check_ranges(op, "mesh", "vert_off", M, vert_off, nv_total, INT_MAX);
    if (rc != LS_OK) return rc;
    rc = check_ranges(op, "mesh", "face_off", M, face_off, nf_total, INT_MAX);
    if (rc != LS_OK) return rc;
    LS_REQUIRE(off_out && r_out, "%s: null off_out / r_out", op);
    std::vector<long long> slot_off(M + 1, 0);
    long long copied_v = 0, copied_f = 0;
    for (int m = 0; m < M; ++m) {
        const long long nv = vert_off[m + 1] - vert_off[m], nf = face_off[m + 1] - face_off[m];
        LS_REQUIRE(nf == 0 || nv > 0, "%s: mesh %d: %lld faces and no vertices", op, m, nf);
        slot_off[m + 1] = slot_off[m] + table_slots(nf, f_target);
        if (nf <= f_target) {   // copied: its size is known here
            copied_v += nv;
            copied_f += nf;
            LS_REQUIRE(!vertices_out || (copied_v <= cap_v && copied_f <= cap_f),
                       "%s: mesh %d: the meshes under the target are copied and do not fit (cap_v %lld, cap_f %lld)", op, m, cap_v, cap_f);
        }
    }
    if (!workspace || workspace_bytes < ls_mesh_cluster_batch_workspace_bytes(M, nv_total, nf_total, r_max)) {
        set_error("%s: workspace too small (need ls_mesh_cluster_batch_workspace_bytes(%d, %lld, %lld, %d))", op, M, nv_total, nf_total, r_max);
        return LS_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const Ws w = layout(workspace, (size_t)OFF_ARRAYS * (M + 1), M, nv_total, nf_total, r_max);
    rc = upload_offsets(w.offs, pack_offsets(M, {vert_off, face_off, slot_off.data()}), st);
    if (rc != LS_OK) return rc;
    return cluster_launch(RaggedMeshes{vertices, faces, w.offs, M, nv_total, nf_total}, M, nv_total, nf_total, (size_t)slot_off[M], f_target, r_max, w,
                          vertices_out, cap_v, faces_out, cap_f, off_out, nullptr, r_out, st);
}

}  // extern "C"

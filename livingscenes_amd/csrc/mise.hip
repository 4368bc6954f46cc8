// mise.hip -- multi-resolution iso-surface extraction (MISE) bookkeeping on the device: which lattice points of the
// (R+1)^3 grid still have to be evaluated by the decoder, and the final dense value grid.
//
// Replaces the CPU octree of
//   /root/reference/lib_shape_prior/core/models/utils/occnet_utils/utils/libmise/mise.pyx            (class MISE)
// as driven by
//   /root/reference/lib_shape_prior/core/models/utils/occnet_utils/mesh_extractor2.py:116-131        (query / eval / update loop)
// (the consumer of the DeepSDF decoder; the reference copies every round's points and values between
// device and host and keeps a std::map keyed octree.)  The reference's pointer octree becomes dense flag arrays:
//   value / known / exists on the lattice, sub[l] = "level-l voxel has been subdivided" (a voxel is a leaf iff all its
//   ancestors are subdivided and it is not).  Per update (mise.pyx:188-236): every KNOWN lattice point marks the leaf voxel
//   of each of its 8 adjacent unit cells as next-to-positive (value >= threshold) and / or next-to-negative (<=); every leaf
//   below the finest level carrying both marks is subdivided and its 27 corner / edge / face / centre points come to exist.
// Everything is integer / flag work plus exact comparisons: the query sets per round and the dense grid are bit-identical to
// the reference's (tests/golden/mise.npz; the ORDER of a round's queries is ascending lattice index instead of the
// reference's insertion order -- the field is point-wise, so it cannot matter).
#include "ls_common.h"
#include "ls_device.h"
#include "ls_scan.h"

namespace ls {

struct MiseLayout {
    int res0, depth, R, G;
    size_t o_val, o_known, o_exists, o_sub[8], o_pos[8], o_neg[8], o_blk, total;   // one octree: offsets from its first byte
    size_t o_batch_blk, batch_total;   // B octrees back to back, `total` bytes each, then the block sums of the batch
    long long npts;
    int nblk;
};
constexpr int MISE_PER_BLOCK = 4096;   // lattice points per compaction workgroup (256 threads x 16)

// The one statement of a MISE state: offsets (an arena over a null base), since every octree of a batch has the same ones.  The block sums of
// a batch, [B][nblk] + the total, follow the B octrees (every octree's own o_blk serves the single ops on that slice).
static MiseLayout mise_layout(int res0, int depth, int B = 1) {
    MiseLayout L{};
    L.res0 = res0; L.depth = depth; L.R = res0 << depth; L.G = L.R + 1;
    L.npts = (long long)L.G * L.G * L.G;
    L.nblk = (int)((L.npts + MISE_PER_BLOCK - 1) / MISE_PER_BLOCK);
    Arena a(nullptr);
    L.o_val = a.take_bytes((size_t)L.npts * 4);
    L.o_known = a.take_bytes((size_t)L.npts);
    L.o_exists = a.take_bytes((size_t)L.npts);
    for (int l = 0; l < depth; ++l) {
        const size_t n = (size_t)(res0 << l) * (res0 << l) * (res0 << l);
        L.o_sub[l] = a.take_bytes(n); L.o_pos[l] = a.take_bytes(n); L.o_neg[l] = a.take_bytes(n);
    }
    L.o_blk = a.take_bytes((size_t)(L.nblk + 1) * 4);
    L.total = a.bytes();
    Arena batch(nullptr);
    batch.take_bytes((size_t)B * L.total);
    L.o_batch_blk = batch.take_bytes(((size_t)B * L.nblk + 1) * 4);
    L.batch_total = batch.bytes();
    return L;
}

struct MiseDev {   // device view passed by value
    float* val; unsigned char* known; unsigned char* exists;
    unsigned char* sub[8]; unsigned char* pos[8]; unsigned char* neg[8];
    int* blk;
    int res0, depth, R, G;
};
static MiseDev mise_dev(void* state, const MiseLayout& L) {
    MiseDev d{};
    char* b = (char*)state;
    d.val = (float*)(b + L.o_val); d.known = (unsigned char*)(b + L.o_known); d.exists = (unsigned char*)(b + L.o_exists);
    for (int l = 0; l < L.depth; ++l) {
        d.sub[l] = (unsigned char*)(b + L.o_sub[l]); d.pos[l] = (unsigned char*)(b + L.o_pos[l]); d.neg[l] = (unsigned char*)(b + L.o_neg[l]);
    }
    d.blk = (int*)(b + L.o_blk);
    d.res0 = L.res0; d.depth = L.depth; d.R = L.R; d.G = L.G;
    return d;
}

// Every kernel below takes a locator by value and asks it which octree its workgroup works on.  MiseDev always views octree 0; octree b
// of a batch lies `stride` bytes further on (a batch state is B single states back to back), so a kernel adds at(b) -- a multiple of 256
// bytes, hence of every element size -- to the view's arrays.  The locator of the single ops holds nothing: instance 0, offset 0, both
// known at compile time, and the launch geometry of one octree.
struct OneGrid {
    __device__ int inst() const { return 0; }
    __device__ int count() const { return 1; }
    __device__ size_t at(int) const { return 0; }
    dim3 grid(int blocks) const { return dim3(blocks); }
};
struct GridBatch {
    int B;
    size_t stride;   // ls_mise_state_bytes(res0, depth)
    __device__ int inst() const { return blockIdx.y; }
    __device__ int count() const { return B; }
    __device__ size_t at(int b) const { return (size_t)b * stride; }
    dim3 grid(int blocks) const { return dim3(blocks, B); }
};
constexpr int MISE_MAX_BATCH = 65535;   // gridDim.y

// initial lattice: the (res0+1)^3 corner points of the coarse voxels exist (mise.pyx:74-85)
template <class Grids>
__global__ void mise_init_kernel(Grids g, MiseDev d, long long npts) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npts) return;
    const size_t o = g.at(g.inst());
    const int G = d.G, z = (int)(i % G), y = (int)((i / G) % G), x = (int)(i / ((long long)G * G));
    const int m = (1 << d.depth) - 1;
    d.exists[o + i] = ((x & m) | (y & m) | (z & m)) == 0;
    d.known[o + i] = 0;
    d.val[o / 4 + i] = 0.f;
}

// ---- query: ordered compaction of exists && !known.  blk = the block sums, [octree][block]: octree after octree, which is the packed
// output order, so ONE scan over all of them yields every block's first output row and, at [b][0], octree b's first row.
template <class Grids>
__global__ __launch_bounds__(256) void mise_count_kernel(Grids g, MiseDev d, long long npts, int* __restrict__ blk) {
    __shared__ int red[4];
    const size_t o = g.at(g.inst());
    const long long base = (long long)blockIdx.x * MISE_PER_BLOCK;
    int c = 0;
    for (int u = 0; u < 16; ++u) {
        const long long i = base + (long long)threadIdx.x * 16 + u;
        if (i < npts) c += (d.exists[o + i] && !d.known[o + i]) ? 1 : 0;
    }
    c = (int)wave_sum((float)c);   // <= 4096: exact in fp32
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) blk[(size_t)g.inst() * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ __launch_bounds__(1024) void mise_scan_kernel(int* blk, int nblk, int* count_out) {   // exclusive scan, one workgroup
    const int total = scan_top_block<int>(blk, nblk);
    if (threadIdx.x == 1023) { blk[nblk] = total; if (count_out) *count_out = total; }
}
template <class Grids>
__global__ __launch_bounds__(256) void mise_emit_kernel(Grids g, MiseDev d, long long npts, const int* __restrict__ blk, float box_size,
                                                        int32_t* __restrict__ idx_out, int32_t* __restrict__ inst_out, float* __restrict__ pts_out,
                                                        long long cap, long long* __restrict__ off_out) {
    __shared__ int wsum[4];
    const int b = g.inst();
    const size_t o = g.at(b);
    const long long base = (long long)blockIdx.x * MISE_PER_BLOCK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned m = 0;
    for (int u = 0; u < 16; ++u) {
        const long long i = base + (long long)tid * 16 + u;
        if (i < npts && d.exists[o + i] && !d.known[o + i]) m |= 1u << u;
    }
    const int c = __builtin_popcount(m);
    int inc = c;   // inclusive scan over the wave
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) { const int v = __shfl_up(inc, k, 64); if (lane >= k) inc += v; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    const size_t first = (size_t)b * gridDim.x;   // the octree's first block sum: its first output row
    if (off_out && blockIdx.x == 0 && tid == 0) {
        off_out[b] = blk[first];
        if (b == g.count() - 1) off_out[b + 1] = blk[(size_t)g.count() * gridDim.x];
    }
    long long off = blk[first + blockIdx.x] + inc - c;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    const int G = d.G;
    for (int u = 0; u < 16; ++u) {
        if (!(m & (1u << u))) continue;
        const long long i = base + (long long)tid * 16 + u;
        if (off < cap) {
            const int z = (int)(i % G), y = (int)((i / G) % G), x = (int)(i / ((long long)G * G));
            idx_out[off] = (int32_t)i;
            if (inst_out) inst_out[off] = b;
            // mesh_extractor2.py:122-124: p / resolution (float32 division), then box_size * (p - 0.5)
            pts_out[(size_t)off * 3 + 0] = box_size * ((float)x / (float)d.R - 0.5f);
            pts_out[(size_t)off * 3 + 1] = box_size * ((float)y / (float)d.R - 0.5f);
            pts_out[(size_t)off * 3 + 2] = box_size * ((float)z / (float)d.R - 0.5f);
        }
        ++off;
    }
}

// ---- update
// one thread per value; its octree is inst[i] (the single op has no inst: octree 0).  A row that names no octree or no lattice point is dropped.
template <class Grids>
__global__ void mise_scatter_kernel(Grids g, MiseDev d, long long npts, const int32_t* __restrict__ idx, const int32_t* __restrict__ inst,
                                    const float* __restrict__ values, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = inst ? inst[i] : 0;
    const long long p = idx[i];
    if ((unsigned)b >= (unsigned)g.count() || p < 0 || p >= npts) return;
    const size_t o = g.at(b);
    d.val[o / 4 + p] = values[i];
    d.known[o + p] = 1;
}
template <class Grids>
__global__ void mise_clear_kernel(Grids g, unsigned char* a, unsigned char* b, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t o = g.at(g.inst());
    if (i < n) { a[o + i] = 0; b[o + i] = 0; }
}
template <class Grids>
__global__ void mise_mark_kernel(Grids g, MiseDev d, long long npts, double threshold) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t o = g.at(g.inst());
    if (i >= npts || !d.known[o + i]) return;
    const int G = d.G, R = d.R, D = d.depth;
    const int z = (int)(i % G), y = (int)((i / G) % G), x = (int)(i / ((long long)G * G));
    const double v = (double)d.val[o / 4 + i];
    const bool ge = v >= threshold, le = v <= threshold;
    for (int di = -1; di <= 0; ++di)
        for (int dj = -1; dj <= 0; ++dj)
            for (int dk = -1; dk <= 0; ++dk) {
                const int px = x + di, py = y + dj, pz = z + dk;
                if (px < 0 || py < 0 || pz < 0 || px >= R || py >= R || pz >= R) continue;
                int l = 0;
                for (; l < D; ++l) {   // descend while the level-l voxel containing the cell is subdivided
                    const int s = D - l, n = d.res0 << l;
                    if (!d.sub[l][o + ((size_t)(px >> s) * n + (py >> s)) * n + (pz >> s)]) break;
                }
                if (l == D) continue;   // finest-level leaves are never subdivided
                const int s = D - l, n = d.res0 << l;
                const size_t c = o + ((size_t)(px >> s) * n + (py >> s)) * n + (pz >> s);
                if (ge) d.pos[l][c] = 1;
                if (le) d.neg[l][c] = 1;
            }
}
template <class Grids>
__global__ void mise_subdivide_kernel(Grids g, MiseDev d, int l) {
    const int n = d.res0 << l;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * n * n) return;
    const size_t o = g.at(g.inst());
    if (!(d.pos[l][o + i] && d.neg[l][o + i])) return;   // marks only ever land on leaves
    d.sub[l][o + i] = 1;
    const int z = (int)(i % n), y = (int)((i / n) % n), x = (int)(i / ((size_t)n * n));
    const int s = d.depth - l, ns = 1 << (s - 1), G = d.G;   // new_size, mise.pyx:245
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            for (int c = 0; c < 3; ++c)
                d.exists[o + ((size_t)((x << s) + a * ns) * G + ((y << s) + b * ns)) * G + ((z << s) + c * ns)] = 1;
}

// ---- dense grid (mise.pyx:128-165); out = [octree][G][G][G]
template <class Grids>
__global__ void mise_dense_fill_kernel(Grids g, MiseDev d, long long npts, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t o = g.at(g.inst());
    if (i < npts) out[(size_t)g.inst() * npts + i] = d.exists[o + i] ? d.val[o / 4 + i] : __builtin_nanf("");
}
template <class Grids>
__global__ void mise_dense_axis_kernel(Grids g, float* __restrict__ out, int G, int axis) {   // one thread per line along `axis`
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= G * G) return;
    out += (size_t)g.inst() * G * G * G;
    const int a = t / G, b = t % G;
    size_t base, stride;
    if (axis == 0) { base = (size_t)a * G + b; stride = (size_t)G * G; }        // (j,k) fixed, walk i
    else if (axis == 1) { base = (size_t)a * G * G + b; stride = (size_t)G; }   // (i,k) fixed, walk j
    else { base = ((size_t)a * G + b) * G; stride = 1; }                        // (i,j) fixed, walk k
    float prev = out[base];
    for (int s = 1; s < G; ++s) {
        const size_t o = base + (size_t)s * stride;
        const float v = out[o];
        if (v != v) out[o] = prev; else prev = v;
    }
}

// ---- launch sequences, written once for both locators
static bool mise_config_ok(int res0, int depth) { return res0 >= 1 && depth >= 0 && depth <= 7 && ((long long)res0 << depth) <= 1024; }

template <class Grids>
static int mise_init_launch(Grids g, const MiseLayout& L, void* state, size_t bytes, hipStream_t st) {
    LS_HIP_CHECK(hipMemsetAsync(state, 0, bytes, st));
    hipLaunchKernelGGL(mise_init_kernel<Grids>, g.grid(cdiv(L.npts, 256)), dim3(256), 0, st, g, mise_dev(state, L), L.npts);
    LS_LAUNCH_CHECK();
    return LS_OK;
}
template <class Grids>
static int mise_query_launch(Grids g, int B, const MiseLayout& L, void* state, int* blk, float box_size, int32_t* idx_out, int32_t* inst_out,
                             float* pts_out, long long cap, int32_t* count_out, long long* off_out, hipStream_t st) {
    const MiseDev d = mise_dev(state, L);
    hipLaunchKernelGGL(mise_count_kernel<Grids>, g.grid(L.nblk), dim3(256), 0, st, g, d, L.npts, blk);
    hipLaunchKernelGGL(mise_scan_kernel, dim3(1), dim3(1024), 0, st, blk, B * L.nblk, count_out);
    hipLaunchKernelGGL(mise_emit_kernel<Grids>, g.grid(L.nblk), dim3(256), 0, st, g, d, L.npts, blk, box_size, idx_out, inst_out, pts_out, cap, off_out);
    LS_LAUNCH_CHECK();
    return LS_OK;
}
template <class Grids>
static int mise_update_launch(Grids g, const MiseLayout& L, void* state, double threshold, const int32_t* idx, const int32_t* inst,
                              const float* values, long long n, hipStream_t st) {
    const MiseDev d = mise_dev(state, L);
    const int res0 = L.res0, depth = L.depth;
    if (n > 0) hipLaunchKernelGGL(mise_scatter_kernel<Grids>, dim3(cdiv(n, 256)), dim3(256), 0, st, g, d, L.npts, idx, inst, values, n);
    for (int l = 0; l < depth; ++l) {
        const size_t nv = (size_t)(res0 << l) * (res0 << l) * (res0 << l);
        hipLaunchKernelGGL(mise_clear_kernel<Grids>, g.grid(cdiv((long long)nv, 256)), dim3(256), 0, st, g, d.pos[l], d.neg[l], nv);
    }
    if (depth > 0) {
        hipLaunchKernelGGL(mise_mark_kernel<Grids>, g.grid(cdiv(L.npts, 256)), dim3(256), 0, st, g, d, L.npts, threshold);
        for (int l = 0; l < depth; ++l) {
            const size_t nv = (size_t)(res0 << l) * (res0 << l) * (res0 << l);
            hipLaunchKernelGGL(mise_subdivide_kernel<Grids>, g.grid(cdiv((long long)nv, 256)), dim3(256), 0, st, g, d, l);
        }
    }
    LS_LAUNCH_CHECK();
    return LS_OK;
}
template <class Grids>
static int mise_dense_launch(Grids g, const MiseLayout& L, void* state, float* grid_out, hipStream_t st) {
    hipLaunchKernelGGL(mise_dense_fill_kernel<Grids>, g.grid(cdiv(L.npts, 256)), dim3(256), 0, st, g, mise_dev(state, L), L.npts, grid_out);
    for (int axis = 0; axis < 3; ++axis)
        hipLaunchKernelGGL(mise_dense_axis_kernel<Grids>, g.grid(cdiv(L.G * L.G, 256)), dim3(256), 0, st, g, grid_out, L.G, axis);
    LS_LAUNCH_CHECK();
    return LS_OK;
}

}  // namespace ls

using namespace ls;

extern "C" {

size_t ls_mise_state_bytes(int res0, int depth) {
    if (!mise_config_ok(res0, depth)) return 0;
    return mise_layout(res0, depth).total;
}
long long ls_mise_lattice_points(int res0, int depth) {
    if (!mise_config_ok(res0, depth)) return 0;
    return mise_layout(res0, depth).npts;
}
size_t ls_mise_batch_state_bytes(int B, int res0, int depth) {
    if (!mise_config_ok(res0, depth) || B < 1 || B > MISE_MAX_BATCH) return 0;
    const MiseLayout L = mise_layout(res0, depth, B);
    if ((long long)B * L.npts >= (1ll << 31)) return 0;
    return L.batch_total;
}

#define MISE_REQUIRE_CONFIG(res0, depth) LS_REQUIRE(mise_config_ok(res0, depth), "mise: resolution_0=%d depth=%d unsupported", res0, depth)
// B octrees per launch: the workgroup's octree is blockIdx.y, and the packed rows of a query are counted in int
#define MISE_REQUIRE_BATCH(B, L)                                                                                                        \
    do {                                                                                                                                \
        LS_REQUIRE((B) >= 1 && (B) <= MISE_MAX_BATCH, "mise: B=%d outside 1..%d", (B), MISE_MAX_BATCH);                                    \
        LS_REQUIRE((long long)(B) * (L).npts < (1ll << 31), "mise: B=%d octrees of %lld lattice points reach 2^31 rows", (B), (L).npts); \
    } while (0)

int ls_mise_init(void* state, size_t state_bytes, int res0, int depth, void* stream) {
    LS_REQUIRE(state != nullptr, "mise: null state");
    MISE_REQUIRE_CONFIG(res0, depth);
    const MiseLayout L = mise_layout(res0, depth);
    if (state_bytes < L.total) { set_error("mise: state %zu < required %zu bytes", state_bytes, L.total); return LS_ERR_WORKSPACE; }
    return mise_init_launch(OneGrid{}, L, state, L.total, (hipStream_t)stream);
}
int ls_mise_init_batch(void* state, size_t state_bytes, int B, int res0, int depth, void* stream) {
    LS_REQUIRE(state != nullptr, "mise: null state");
    MISE_REQUIRE_CONFIG(res0, depth);
    const MiseLayout L = mise_layout(res0, depth, B);
    MISE_REQUIRE_BATCH(B, L);
    if (state_bytes < L.batch_total) { set_error("mise: batch state %zu < required %zu bytes", state_bytes, L.batch_total); return LS_ERR_WORKSPACE; }
    return mise_init_launch(GridBatch{B, L.total}, L, state, L.batch_total, (hipStream_t)stream);
}

// Unknown lattice points in ascending lattice order: idx_out[cap] (linear index (x*G + y)*G + z), pts_out[cap,3] (the
// decoder's query coordinates, mesh_extractor2.py:122-124), *count_out (device int; may exceed cap: nothing past cap is written).
int ls_mise_query(void* state, int res0, int depth, float box_size, int32_t* idx_out, float* pts_out, int cap, int32_t* count_out,
                  void* stream) {
    LS_REQUIRE(state && idx_out && pts_out && count_out && cap >= 0, "mise_query: null argument");
    MISE_REQUIRE_CONFIG(res0, depth);
    const MiseLayout L = mise_layout(res0, depth);
    return mise_query_launch(OneGrid{}, 1, L, state, mise_dev(state, L).blk, box_size, idx_out, nullptr, pts_out, cap, count_out, nullptr,
                             (hipStream_t)stream);
}
// The same for B octrees: octree 0's points first, then octree 1's ...; inst_out = the octree of each row; off_out (DEVICE [B+1]) = the
// first row of every octree and the total, always the full counts.
int ls_mise_query_batch(void* state, int B, int res0, int depth, float box_size, int32_t* idx_out, int32_t* inst_out, float* pts_out,
                        long long cap, long long* off_out, void* stream) {
    LS_REQUIRE(state && idx_out && inst_out && pts_out && off_out && cap >= 0, "mise_query_batch: null argument");
    MISE_REQUIRE_CONFIG(res0, depth);
    const MiseLayout L = mise_layout(res0, depth, B);
    MISE_REQUIRE_BATCH(B, L);
    return mise_query_launch(GridBatch{B, L.total}, B, L, state, (int*)((char*)state + L.o_batch_blk), box_size, idx_out, inst_out, pts_out,
                             cap, nullptr, off_out, (hipStream_t)stream);
}

// Store the values of the queried points, then subdivide every active leaf voxel (mise.pyx:87-102, 188-236).
int ls_mise_update(void* state, int res0, int depth, double threshold, const int32_t* idx, const float* values, int n, void* stream) {
    LS_REQUIRE(state && (n == 0 || (idx && values)) && n >= 0, "mise_update: null argument");
    MISE_REQUIRE_CONFIG(res0, depth);
    return mise_update_launch(OneGrid{}, mise_layout(res0, depth), state, threshold, idx, nullptr, values, n, (hipStream_t)stream);
}
// The same for B octrees: row i belongs to octree inst[i].  An octree without rows is updated too; for one whose query came back empty
// that changes nothing (its last update subdivided no voxel, so marking again finds the same marks).
int ls_mise_update_batch(void* state, int B, int res0, int depth, double threshold, const int32_t* idx, const int32_t* inst, const float* values,
                         long long n, void* stream) {
    LS_REQUIRE(state && (n == 0 || (idx && inst && values)) && n >= 0, "mise_update_batch: null argument");
    MISE_REQUIRE_CONFIG(res0, depth);
    const MiseLayout L = mise_layout(res0, depth);
    MISE_REQUIRE_BATCH(B, L);
    LS_REQUIRE(n <= (long long)B * L.npts, "mise_update_batch: %lld values for %d octrees of %lld lattice points", n, B, L.npts);
    return mise_update_launch(GridBatch{B, L.total}, L, state, threshold, idx, inst, values, n, (hipStream_t)stream);
}

// Dense (R+1)^3 value grid: known values, the rest completed along x, then y, then z (mise.pyx:128-165).
int ls_mise_to_dense(void* state, int res0, int depth, float* grid_out, void* stream) {
    LS_REQUIRE(state && grid_out, "mise_to_dense: null argument");
    MISE_REQUIRE_CONFIG(res0, depth);
    return mise_dense_launch(OneGrid{}, mise_layout(res0, depth), state, grid_out, (hipStream_t)stream);
}
int ls_mise_to_dense_batch(void* state, int B, int res0, int depth, float* grid_out, void* stream) {
    LS_REQUIRE(state && grid_out, "mise_to_dense_batch: null argument");
    MISE_REQUIRE_CONFIG(res0, depth);
    const MiseLayout L = mise_layout(res0, depth);
    MISE_REQUIRE_BATCH(B, L);
    return mise_dense_launch(GridBatch{B, L.total}, L, state, grid_out, (hipStream_t)stream);
}

}  // extern "C"

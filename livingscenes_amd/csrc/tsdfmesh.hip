// tsdfmesh.hip -- scene memory: the fused state of an instance (depthfuse.hip: sum, n) meshed where it was OBSERVED.  Marching cubes at
// isovalue 0 of D = fuse_value(sum, n), restricted to the cubes whose eight corners are valid samples, with only the vertices those
// cubes name: tests/fuse_oracle.py: mesh, vertices and faces alike.  The definition is in include/livingscenes_hip.h (ls_tsdf_mesh_f64);
// the arithmetic of every step is tsdfmesh_plan.h, which tests/tools/tsdfmesh_plan_run.cpp runs on the host to the same arrays.  This
// file shares no kernel, launch sequence, constant table or upload flag with mcubes.hip, materialises no float64 volume and has no
// compaction step: whether a vertex is used is a local rule on the kept bits (mesh_carried), so the scan numbers the final vertices
// and the face pass writes final indices.  What this file adds, one launch per pass whatever P (all problems of a call share the dims;
// the problem is blockIdx.y):
//   classify   a workgroup owns 4096 consecutive SAMPLES, consecutive k on consecutive lanes: the thread of sample (i, j, k) with i, j, k
//              below the cube counts gathers the eight (sum, n) of cube (i, j, k) -> class (pattern | kept << 8, 16 bit); the optional
//              statistics are summed per workgroup: three integer atomics each
//   count      a workgroup owns 4096 consecutive cubes, a thread 16: the carried mask of each (kept bits of up to six neighbours) is
//              stored, the packed counts (vertices << 32 | face indices) are summed per workgroup
//   scan       scan_top_block (ls_scan.h) over the workgroup sums of the whole batch: the packed output order
//   vertices   per-cube bases by a scan inside the workgroup, stored where the face pass will read them (a cube with a carried vertex, a
//              cube with a face); the carried vertices of every cube; the offsets of the batch
//   faces      one thread per cube; a kept cube writes its final indices
// No allocation, no host synchronisation, no floating-point atomics; hipGetLastError() after every launch, the pass named.
#include <cmath>
#include <vector>

#include "ls_common.h"
#include "ls_scan.h"
#include "ls_workspace.h"

// the arithmetic of the definition as written: no contraction of a * b + c into an fma anywhere in this file
#pragma clang fp contract(off)
#include "tsdfmesh_plan.h"

namespace ls {
namespace tmk {
using namespace tm;

struct MeshArgs {
    const int* sum;                // [P,nx,ny,nz]
    const int* n;                  // [P,nx,ny,nz]
    MeshDims d;
    int P, min_obs, nblk;
    const double* grids;           // [P,4]: origin, voxel, in the workspace
    unsigned short* cls;           // [P,ncubes]
    unsigned short* carried;       // [P,ncubes]
    int* vbase;                    // [P,ncubes]
    int* pbase;                    // [P,ncubes]
    u64* blk;                      // [P,nblk] + the total
    double* vertices;              // packed [.,3], may be null
    long long cap_v;
    long long* faces;              // packed indices, may be null
    long long cap_idx;             // 3 cap_f
    long long* off_out;            // [2][P+1]
    long long* stats;              // [P,3], may be null
};

// pass 1: a workgroup owns 4096 consecutive samples of problem blockIdx.y, a thread every 256th of them: consecutive k on consecutive lanes.
// The statistics are summed in registers (three 20-bit fields of one word: at most 4096 each), then per wave and per workgroup: three
// integer atomics per workgroup -- one per wave and field was measured at 1.5 ms of same-address atomics on 64 x 64^3 samples.
__global__ __launch_bounds__(MESH_CHUNK) void tsdfmesh_classify_kernel(MeshArgs G) {
    __shared__ u64 red[MESH_CHUNK / kWave];
    const int p = blockIdx.y;
    const int* sum = G.sum + (size_t)p * G.d.samples;
    const int* n = G.n + (size_t)p * G.d.samples;
    const unsigned nz = (unsigned)G.d.sz, ny = (unsigned)G.d.sy;
    u64 acc = 0;                                                             // valid | kept << 20 | dropped with a crossing << 40
    for (int it = 0; it < MESH_ITEMS; ++it) {
        const long long s = (long long)blockIdx.x * MESH_PER_BLOCK + (long long)it * MESH_CHUNK + threadIdx.x;
        if (s >= G.d.samples) break;
        const unsigned u = (unsigned)s;                                      // s < 2^31
        const int k = (int)(u % nz), j = (int)((u / nz) % ny), i = (int)((u / nz) / ny);
        acc += (u64)(n[s] >= G.min_obs);
        if (i < G.d.cx && j < G.d.cy && k < G.d.cz) {
            const unsigned c = mesh_classify(sum, n, G.d, i, j, k, G.min_obs);
            G.cls[(size_t)p * G.d.ncubes + mesh_cube_index(G.d, i, j, k)] = (unsigned short)c;
            const bool kept = (c & MESH_KEPT_BIT) != 0;
            acc += (u64)kept << 20;
            acc += (u64)(!kept && (c & 255u) != 0 && (c & 255u) != 255u) << 40;
        }
    }
    if (!G.stats) return;                                                    // the whole workgroup
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);       // at most 4096 per field in a workgroup: no field carries
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 t = red[0] + red[1] + red[2] + red[3];
        unsigned long long* st = (unsigned long long*)(G.stats + (size_t)p * MESH_FIELDS);
        const u64 field = (1ull << 20) - 1;
        if (t & field) atomicAdd(st + MESH_VALID, t & field);
        if ((t >> 20) & field) atomicAdd(st + MESH_KEPT, (t >> 20) & field);
        if ((t >> 40) & field) atomicAdd(st + MESH_DROPPED_CROSSED, (t >> 40) & field);
    }
}

// pass 2: the carried mask per cube, the packed counts summed per workgroup
__global__ __launch_bounds__(MESH_CHUNK) void tsdfmesh_count_kernel(MeshArgs G) {
    __shared__ u64 red[MESH_CHUNK / kWave];
    const int p = blockIdx.y;
    const unsigned short* cls = G.cls + (size_t)p * G.d.ncubes;
    unsigned short* carried = G.carried + (size_t)p * G.d.ncubes;
    const long long base = (long long)blockIdx.x * MESH_PER_BLOCK + (long long)threadIdx.x * MESH_ITEMS;
    u64 acc = 0;
    for (int u = 0; u < MESH_ITEMS; ++u) {
        const long long c = base + u;
        if (c >= G.d.ncubes) break;
        int i, j, k;
        mesh_cube_ijk(G.d, c, &i, &j, &k);
        const unsigned m = mesh_carried(cls, G.d, i, j, k);
        carried[c] = (unsigned short)m;
        acc += mesh_counts(cls[c], m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) G.blk[(size_t)p * G.nblk + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// pass 3: exclusive scan of the workgroup sums of the whole batch (one workgroup); the total -> blk[count]
__global__ __launch_bounds__(1024) void tsdfmesh_scan_kernel(u64* blk, int count) {
    const u64 total = scan_top_block<u64>(blk, count);
    if (threadIdx.x == 1023) blk[count] = total;
}

// pass 4: per-cube bases (both count from the start of the packed output), the vertices, and the offsets of the batch:
// off_out[p] = first vertex of mesh p, off_out[P + 1 + p] = its first face, [P] and [2 P + 1] the totals
__global__ __launch_bounds__(MESH_CHUNK) void tsdfmesh_vertex_kernel(MeshArgs G) {
    __shared__ u64 wsum[MESH_CHUNK / kWave];
    const int p = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const unsigned short* cls = G.cls + (size_t)p * G.d.ncubes;
    const unsigned short* carried = G.carried + (size_t)p * G.d.ncubes;
    int* vbase = G.vbase + (size_t)p * G.d.ncubes;
    int* pbase = G.pbase + (size_t)p * G.d.ncubes;
    const size_t first = (size_t)p * G.nblk;                        // the problem's first workgroup sum: where its mesh starts
    if (blockIdx.x == 0 && tid == 0) {
        G.off_out[p] = (long long)(G.blk[first] >> 32);
        G.off_out[G.P + 1 + p] = (long long)(G.blk[first] & 0xFFFFFFFFull) / 3;
        if (p == G.P - 1) {
            const u64 total = G.blk[(size_t)G.P * G.nblk];
            G.off_out[G.P] = (long long)(total >> 32);
            G.off_out[2 * G.P + 1] = (long long)(total & 0xFFFFFFFFull) / 3;
        }
    }
    const long long base = (long long)blockIdx.x * MESH_PER_BLOCK + (long long)tid * MESH_ITEMS;
    u64 mine = 0;
    for (int u = 0; u < MESH_ITEMS; ++u) {
        const long long c = base + u;
        if (c >= G.d.ncubes) break;
        mine += mesh_counts(cls[c], carried[c]);
    }
    u64 inc = mine;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) { const u64 v = __shfl_up(inc, o, kWave); if (lane >= o) inc += v; }
    if (lane == kWave - 1) wsum[wave] = inc;
    __syncthreads();
    u64 run = G.blk[first + blockIdx.x] + inc - mine;
    for (int w = 0; w < wave; ++w) run += wsum[w];
    const int* sum = G.sum + (size_t)p * G.d.samples;
    const int* n = G.n + (size_t)p * G.d.samples;
    const double* g = G.grids + (size_t)p * 4;
    const double origin[3] = {g[0], g[1], g[2]};
    const double voxel = g[3];
    for (int u = 0; u < MESH_ITEMS; ++u) {
        const long long c = base + u;
        if (c >= G.d.ncubes) break;
        const unsigned m = carried[c];
        const long long vb = (long long)(run >> 32);
        const u64 cnt = mesh_counts(cls[c], m);
        if (m) vbase[c] = (int)vb;                                            // read by the face pass only for a cube with a carried vertex ...
        if (cnt & 0xFFFFFFFFull) pbase[c] = (int)(run & 0xFFFFFFFFull);       // ... and only for a cube with a face: most cubes have neither
        if (m && G.vertices) {
            int i, j, k;
            mesh_cube_ijk(G.d, c, &i, &j, &k);
            mesh_emit_vertices(sum, n, G.d, G.min_obs, origin, voxel, i, j, k, m, vb, G.vertices, G.cap_v);
        }
        run += cnt;
    }
}

// pass 5: the faces of the kept cubes; their indices count from the mesh's own first vertex
__global__ __launch_bounds__(MESH_CHUNK) void tsdfmesh_face_kernel(MeshArgs G) {
    const long long c = (long long)blockIdx.x * MESH_CHUNK + threadIdx.x;
    if (c >= G.d.ncubes) return;
    const int p = blockIdx.y;
    const unsigned short* cls = G.cls + (size_t)p * G.d.ncubes;
    const unsigned cl = cls[c];
    if (!(cl & MESH_KEPT_BIT) || (cl & 255u) == 0 || (cl & 255u) == 255u) return;
    const long long v0 = (long long)(G.blk[(size_t)p * G.nblk] >> 32);
    int i, j, k;
    mesh_cube_ijk(G.d, c, &i, &j, &k);
    mesh_emit_faces(cls, G.carried + (size_t)p * G.d.ncubes, G.vbase + (size_t)p * G.d.ncubes, G.d, i, j, k, (long long)G.pbase[(size_t)p * G.d.ncubes + c],
                    v0, G.faces, G.cap_idx);
}

}  // namespace tmk
}  // namespace ls

using namespace ls;
using namespace ls::tmk;

namespace {
struct Ws {
    unsigned short* cls; unsigned short* carried; int* vbase; int* pbase; u64* blk; double* grids;
    int nblk;
    size_t bytes;
};

// the one layout: the pieces of tsdfmesh_plan.h from one Arena (ws null: a sizing pass)
Ws layout(void* ws, int P, int nx, int ny, int nz) {
    const MeshPieces c = mesh_pieces(P, nx, ny, nz);
    Arena ar(ws);
    Ws w;
    w.cls = ar.take<unsigned short>(c.cubes);
    w.carried = ar.take<unsigned short>(c.cubes);
    w.vbase = ar.take<int>(c.cubes);
    w.pbase = ar.take<int>(c.cubes);
    w.blk = ar.take<u64>(c.sums);
    w.grids = ar.take<double>(c.grid_words);
    w.nblk = c.nblk;
    w.bytes = ar.bytes();
    return w;
}

size_t workspace_need(int P, int nx, int ny, int nz) {
    if (mesh_bad_sizes(P, nx, ny, nz)) return 0;
    if (nx < 2 || ny < 2 || nz < 2) return kWorkspaceAlign;
    return layout(nullptr, P, nx, ny, nz).bytes;
}

#define LS_MESH_PASS(name)                                                                                   \
    do {                                                                                                     \
        hipError_t _e = hipGetLastError();                                                                   \
        if (_e != hipSuccess) {                                                                              \
            ls::set_error("%s: the %s pass failed to launch: %s (%s:%d)", op, name, hipGetErrorString(_e), __FILE__, __LINE__); \
            return LS_ERR_HIP;                                                                               \
        }                                                                                                    \
    } while (0)

// everything the host decides, then the copy of the grids and the passes
int mesh_run(const char* op, int P, const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, const double* voxel,
             double* vertices, long long cap_v, long long* faces, long long cap_f, long long* off_out, long long* stats, void* workspace,
             size_t workspace_bytes, hipStream_t st) {
    const int bad = mesh_bad_sizes(P, nx, ny, nz);
    LS_REQUIRE(bad != 1, "%s: dims must be at least 1, got %d x %d x %d", op, nx, ny, nz);
    LS_REQUIRE(bad != 2, "%s: P = %d outside 1..%d", op, P, MESH_MAX_BATCH);
    LS_REQUIRE(bad != 3, "%s: 15 * P * nx * ny * nz = 15 * %d * %d * %d * %d reaches 2^31 (int vertex and face bases)", op, P, nx, ny, nz);
    LS_REQUIRE(min_obs >= 1, "%s: min_obs must be >= 1 (a sample never observed has no distance), got %d", op, min_obs);
    LS_REQUIRE(sum && n && off_out, "%s: null sum / n / off_out", op);
    LS_REQUIRE(origin && voxel, "%s: null origin / voxel", op);
    for (int p = 0; p < P; ++p) {
        const int g = fp::fuse_bad_grid(origin + (size_t)p * 3, voxel[p], 1.0);
        LS_REQUIRE(g != 1, "%s: problem %d: origin must be finite, got (%g, %g, %g)", op, p, origin[p * 3], origin[p * 3 + 1], origin[p * 3 + 2]);
        LS_REQUIRE(g != 2, "%s: problem %d: voxel must be finite and > 0, got %g", op, p, voxel[p]);
    }
    LS_REQUIRE(cap_v >= 0 && cap_f >= 0, "%s: negative capacity (cap_v = %lld, cap_f = %lld)", op, cap_v, cap_f);
    LS_REQUIRE((vertices == nullptr) == (faces == nullptr), "%s: vertices and faces are given together, or both null (a sizing call)", op);
    const size_t need = workspace_need(P, nx, ny, nz);
    if (!(workspace && workspace_bytes >= need)) {
        set_error("%s: workspace %zu < required %zu (ls_%s_workspace_bytes)", op, workspace ? workspace_bytes : (size_t)0, need, op);
        return LS_ERR_WORKSPACE;
    }
    if (stats) LS_HIP_CHECK(hipMemsetAsync(stats, 0, (size_t)P * MESH_FIELDS * sizeof(long long), st));
    if (nx < 2 || ny < 2 || nz < 2) {                                         // no cube: empty meshes (the valid samples are still counted below)
        LS_HIP_CHECK(hipMemsetAsync(off_out, 0, (size_t)(2 * P + 2) * sizeof(long long), st));
        if (!stats) return LS_OK;
    }
    const Ws w = layout(workspace, P, nx, ny, nz);
    MeshArgs G{};
    G.sum = sum; G.n = n;
    G.d = mesh_dims(nx, ny, nz);
    G.P = P; G.min_obs = min_obs; G.nblk = w.nblk;
    G.stats = stats;
    const dim3 threads(MESH_CHUNK);
    if (G.d.ncubes == 0) {                                                    // only the valid samples: no cube is touched, nothing of the workspace is used
        hipLaunchKernelGGL(tsdfmesh_classify_kernel, dim3((unsigned)cdiv(G.d.samples, MESH_PER_BLOCK), (unsigned)P), threads, 0, st, G);
        LS_MESH_PASS("classify");
        return LS_OK;
    }
    std::vector<double> grids((size_t)P * 4);
    for (int p = 0; p < P; ++p) {
        for (int a = 0; a < 3; ++a) grids[(size_t)p * 4 + a] = origin[(size_t)p * 3 + a];
        grids[(size_t)p * 4 + 3] = voxel[p];
    }
    LS_HIP_CHECK(hipMemcpyAsync(w.grids, grids.data(), grids.size() * sizeof(double), hipMemcpyHostToDevice, st));   // pageable: read when it returns
    G.grids = w.grids;
    G.cls = w.cls; G.carried = w.carried; G.vbase = w.vbase; G.pbase = w.pbase; G.blk = w.blk;
    G.vertices = vertices; G.cap_v = cap_v;
    G.faces = faces; G.cap_idx = cap_f * 3;
    G.off_out = off_out;
    hipLaunchKernelGGL(tsdfmesh_classify_kernel, dim3((unsigned)cdiv(G.d.samples, MESH_PER_BLOCK), (unsigned)P), threads, 0, st, G);
    LS_MESH_PASS("classify");
    hipLaunchKernelGGL(tsdfmesh_count_kernel, dim3((unsigned)w.nblk, (unsigned)P), threads, 0, st, G);
    LS_MESH_PASS("count");
    hipLaunchKernelGGL(tsdfmesh_scan_kernel, dim3(1), dim3(1024), 0, st, w.blk, P * w.nblk);
    LS_MESH_PASS("scan");
    hipLaunchKernelGGL(tsdfmesh_vertex_kernel, dim3((unsigned)w.nblk, (unsigned)P), threads, 0, st, G);
    LS_MESH_PASS("vertex");
    if (faces) {
        hipLaunchKernelGGL(tsdfmesh_face_kernel, dim3((unsigned)cdiv(G.d.ncubes, MESH_CHUNK), (unsigned)P), threads, 0, st, G);
        LS_MESH_PASS("face");
    }
    return LS_OK;
}
}  // namespace

extern "C" {

size_t ls_tsdf_mesh_workspace_bytes(int nx, int ny, int nz) { return workspace_need(1, nx, ny, nz); }
size_t ls_tsdf_mesh_batch_workspace_bytes(int P, int nx, int ny, int nz) { return workspace_need(P, nx, ny, nz); }

int ls_tsdf_mesh_f64(const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, double voxel, double* vertices,
                     long long cap_v, long long* faces, long long cap_f, long long* off_out, long long* stats_out, void* workspace, size_t workspace_bytes,
                     void* stream) {
    return mesh_run("tsdf_mesh", 1, sum, n, nx, ny, nz, min_obs, origin, &voxel, vertices, cap_v, faces, cap_f, off_out, stats_out, workspace,
                    workspace_bytes, (hipStream_t)stream);
}

int ls_tsdf_mesh_batch_f64(int P, const int32_t* sum, const int32_t* n, int nx, int ny, int nz, int min_obs, const double* origin, const double* voxel,
                           double* vertices, long long cap_v, long long* faces, long long cap_f, long long* off_out, long long* stats_out,
                           void* workspace, size_t workspace_bytes, void* stream) {
    return mesh_run("tsdf_mesh_batch", P, sum, n, nx, ny, nz, min_obs, origin, voxel, vertices, cap_v, faces, cap_f, off_out, stats_out, workspace,
                    workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"

// tsdfmesh_plan_run -- csrc/tsdfmesh_plan.h compiled on its own with the host compiler and run to the END: the five passes of
// csrc/tsdfmesh.hip (classify, count, exclusive scan of the workgroup sums, vertices, faces) one after the other, sequentially, with the
// header's functions -- the same functions the kernels call, over the same per-cube arrays and workgroup sums.  For
// tests/test_tsdf_mesh_cpu.py, which holds the output to tests/fuse_oracle.py: mesh by equality.
// stdin, whitespace separated: nx ny nz min_obs origin[3] voxel (C99 hexadecimal doubles), then sum[nx ny nz] and n[nx ny nz] (k fastest).
// A first token "constants" instead answers MESH_CHUNK MESH_ITEMS MESH_PER_BLOCK MESH_MAX_BATCH and ends.
// stdout: "nv nf kept dropped_crossed valid", then nv lines of three hexadecimal doubles, then nf lines of three indices.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "tsdfmesh_plan.h"

int main() {
    using namespace ls::tm;
    std::string tok;
    if (!(std::cin >> tok)) return 2;
    if (tok == "constants") {
        printf("%d %d %d %d\n", MESH_CHUNK, MESH_ITEMS, MESH_PER_BLOCK, MESH_MAX_BATCH);
        return 0;
    }
    const int nx = atoi(tok.c_str());
    int ny, nz, min_obs;
    if (!(std::cin >> ny >> nz >> min_obs)) return 2;
    double grid[4];
    for (double& g : grid) {
        if (!(std::cin >> tok)) return 2;
        g = strtod(tok.c_str(), nullptr);
    }
    if (mesh_bad_sizes(1, nx, ny, nz) || min_obs < 1 || ls::fp::fuse_bad_grid(grid, grid[3], 1.0)) return 3;
    const MeshDims d = mesh_dims(nx, ny, nz);
    std::vector<int> sum((size_t)d.samples), n((size_t)d.samples);
    for (int& v : sum) if (!(std::cin >> v)) return 2;
    for (int& v : n) if (!(std::cin >> v)) return 2;
    long long stats[MESH_FIELDS] = {0, 0, 0};
    for (int v : n) stats[MESH_VALID] += v >= min_obs;
    if (nx < 2 || ny < 2 || nz < 2) {
        printf("0 0 0 0 %lld\n", stats[MESH_VALID]);
        return 0;
    }
    const MeshPieces pc = mesh_pieces(1, nx, ny, nz);
    std::vector<unsigned short> cls(pc.cubes), carried(pc.cubes);
    std::vector<int> vbase(pc.cubes, -1), pbase(pc.cubes, -1);               // stored as the vertex pass stores them: only where the face pass reads
    std::vector<u64> blk(pc.sums, 0);
    // classify
    for (long long c = 0; c < d.ncubes; ++c) {
        int i, j, k;
        mesh_cube_ijk(d, c, &i, &j, &k);
        if (mesh_cube_index(d, i, j, k) != c) return 4;
        const unsigned cl = mesh_classify(sum.data(), n.data(), d, i, j, k, min_obs);
        cls[(size_t)c] = (unsigned short)cl;
        const bool kept = (cl & MESH_KEPT_BIT) != 0;
        stats[MESH_KEPT] += kept;
        stats[MESH_DROPPED_CROSSED] += !kept && (cl & 255u) != 0 && (cl & 255u) != 255u;
    }
    // count: the carried masks, the packed counts per workgroup
    for (long long c = 0; c < d.ncubes; ++c) {
        int i, j, k;
        mesh_cube_ijk(d, c, &i, &j, &k);
        const unsigned m = mesh_carried(cls.data(), d, i, j, k);
        carried[(size_t)c] = (unsigned short)m;
        blk[(size_t)(c / MESH_PER_BLOCK)] += mesh_counts(cls[(size_t)c], m);
    }
    // scan: exclusive, the total behind the last sum
    u64 run = 0;
    for (int b = 0; b < pc.nblk; ++b) {
        const u64 v = blk[(size_t)b];
        blk[(size_t)b] = run;
        run += v;
    }
    blk[(size_t)pc.nblk] = run;
    const long long nv = (long long)(run >> 32), nidx = (long long)(run & 0xFFFFFFFFull);
    if (nidx % 3) return 5;
    // -1 and NaN below the counts would show an entry no pass wrote
    std::vector<double> vertices((size_t)nv * 3, __builtin_nan(""));
    std::vector<long long> faces((size_t)nidx, -1);
    // vertices: the per-cube bases, the carried vertices
    for (int b = 0; b < pc.nblk; ++b) {
        u64 at = blk[(size_t)b];
        for (long long c = (long long)b * MESH_PER_BLOCK; c < d.ncubes && c < (long long)(b + 1) * MESH_PER_BLOCK; ++c) {
            int i, j, k;
            mesh_cube_ijk(d, c, &i, &j, &k);
            const u64 cnt = mesh_counts(cls[(size_t)c], carried[(size_t)c]);
            if (carried[(size_t)c]) vbase[(size_t)c] = (int)(at >> 32);
            if (cnt & 0xFFFFFFFFull) pbase[(size_t)c] = (int)(at & 0xFFFFFFFFull);
            mesh_emit_vertices(sum.data(), n.data(), d, min_obs, grid, grid[3], i, j, k, carried[(size_t)c], (long long)(at >> 32), vertices.data(), nv);
            at += cnt;
        }
    }
    // faces
    const long long v0 = (long long)(blk[0] >> 32);
    for (long long c = 0; c < d.ncubes; ++c) {
        if (!(cls[(size_t)c] & MESH_KEPT_BIT)) continue;
        int i, j, k;
        mesh_cube_ijk(d, c, &i, &j, &k);
        mesh_emit_faces(cls.data(), carried.data(), vbase.data(), d, i, j, k, pbase[(size_t)c], v0, faces.data(), nidx);
    }
    printf("%lld %lld %lld %lld %lld\n", nv, nidx / 3, stats[MESH_KEPT], stats[MESH_DROPPED_CROSSED], stats[MESH_VALID]);
    for (long long v = 0; v < nv; ++v) printf("%a %a %a\n", vertices[(size_t)v * 3], vertices[(size_t)v * 3 + 1], vertices[(size_t)v * 3 + 2]);
    for (long long f = 0; f < nidx / 3; ++f) printf("%lld %lld %lld\n", faces[(size_t)f * 3], faces[(size_t)f * 3 + 1], faces[(size_t)f * 3 + 2]);
    return 0;
}

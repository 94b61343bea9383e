// isosurface_kernels.h -- launch interface of the marching-tetrahedra kernels behind nerf_isosurface_grid / nerf_extract_mesh (internal).
//
// The conventions of the output (lattice, inside predicate, vertex and triangle order, winding, canonical form, normals) are those of
// include/nerf_mi355x.h, "isosurface meshes"; isosurface_kernels.hip restates how each kernel meets them.
//
// Workspace: 16 bytes per lattice point (sigma f32, the classification word, the two exclusive prefix sums) plus 8 bytes per 256 points
// (the block sums of the scan) plus a 256-byte header: 268 MB for 256^3.  The outputs are not part of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct MeshLattice {
    int nx, ny, nz;       // every one >= 2; nx * ny * nz <= 2^28
    float lo[3], step[3]; // p = lo + step * index, product and sum each rounded once
    float iso;
};

constexpr int kMeshScanBlock = 256; // lattice points per block of the scan (= threads per workgroup of every kernel here)

struct MeshWorkspace {
    uint32_t *totals; // {n_vertices, n_triangles}
    float *sigma;     // n points, x fastest
    uint32_t *info;   // per point: bits 1..7 edge mask (bit dx + 2 dy + 4 dz), bits 8..15 inside mask of the cell's corners, bits 16..19 triangles of the cell
    uint32_t *vbase;  // exclusive prefix sum of popcount(edge mask): first vertex id of the point
    uint32_t *tbase;  // exclusive prefix sum of the triangle counts: first triangle of the cell whose low corner the point is
    uint32_t *vsum, *tsum; // per scan block: its two sums, then (in place) their exclusive prefix sums
    uint32_t n_points, n_blocks;
};

size_t mesh_workspace_bytes(size_t n_points);
MeshWorkspace mesh_workspace_carve(void *base, size_t n_points);

// classify -> block sums -> scan of the block sums (one workgroup): w.totals holds both counts when these three launches have run.
// label / size (both or neither; components_kernels.h): the filtered classification -- a point whose component lacks the keep bit is not inside.
hipError_t launch_mesh_count(const MeshLattice &g, const MeshWorkspace &w, hipStream_t st, const uint32_t *label = nullptr, const uint32_t *size = nullptr);
// add (vbase, tbase) -> vertices -> triangles.  Every output is optional (device pointers):
//   vertices, normals  n_vertices x 3 floats;  pts_soa  3 x n_vertices floats (x row, y row, z row);  neg_normals  n_vertices x 3 floats (-normal:
//   the view direction that looks at the surface head-on);  triangles  n_triangles x 3 vertex ids
hipError_t launch_mesh_emit(const MeshLattice &g, const MeshWorkspace &w, uint32_t n_vertices, float *vertices, float *normals, float *pts_soa,
                            float *neg_normals, uint32_t n_triangles, uint32_t *triangles, hipStream_t st);

// components_kernels.h -- launch interface of the connected-component kernels behind nerf_lattice_components and the filtered mesh entry
// points (internal).  The definition (inside predicate, the 14 Kuhn neighbours, label = smallest linear index, rank order, filter) is that of
// include/nerf_mi355x.h, "lattice components"; components_kernels.hip restates how each kernel meets it.
//
// Workspace: 8 bytes per lattice point (the label, and one word that holds the component's size at its root plus the keep flag) plus 4 bytes per
// 256 points (block sums of the root scan) plus a 4 KiB header (counts, the ranking's winners, the table).  Two further words per point are
// only needed between labelling and classification -- the compacted list of roots and the root -> rank map -- and are borrowed from the mesh
// workspace (vbase, tbase), which is idle until k_mesh_scan_add runs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr uint32_t kCompNone = 0xFFFFFFFFu; // label of a point that is not inside
constexpr uint32_t kCompKeepBit = 0x80000000u; // in size[root]: the component passes the filter (sizes are at most 2^28)
constexpr int kCompMaxRank = 64;             // largest keep_largest / cap_table

struct CompEntry { uint32_t label, n_points; int32_t bounds[6]; }; // = nerf_component

struct CompWorkspace {
    uint32_t *counts;          // {n_components, n_kept}
    unsigned long long *win;   // kCompMaxRank keys (n_points << 32) | (0xFFFFFFFF - label) in rank order, 0 = no such component
    CompEntry *table;          // kCompMaxRank entries
    uint32_t *label;           // per point
    uint32_t *size;            // per point, meaningful at roots: n_points | kCompKeepBit
    uint32_t *bsum;            // per block of 256 points: roots in the block, then (in place) the exclusive prefix sums
    uint32_t *roots, *rankmap; // borrowed, n_points words each: the roots in ascending order; per root its rank or kCompNone
    uint32_t n_points, n_blocks;
};

size_t comp_workspace_bytes(size_t n_points);
CompWorkspace comp_workspace_carve(void *base, size_t n_points, uint32_t *roots, uint32_t *rankmap);

// label -> flatten -> sizes -> root scan -> rank (max(keep_largest, cap_table) arg-max passes) -> keep flags [-> table + bounds when cap_table > 0].
// sigma: nx * ny * nz floats on the device, x fastest.  keep_largest, cap_table <= kCompMaxRank.  When the launches have run, w.counts, w.label,
// w.size (keep bits) and the first cap_table entries of w.table are final.
hipError_t launch_components(const float *sigma, int nx, int ny, int nz, float iso, const CompWorkspace &w, uint32_t keep_largest, uint32_t min_points,
                             uint32_t cap_table, hipStream_t st);

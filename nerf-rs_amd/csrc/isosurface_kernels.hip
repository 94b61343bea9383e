// isosurface_kernels.hip -- marching tetrahedra on the Kuhn split of a sigma lattice: the level set sigma = iso as a deterministic, welded,
// indexed triangle mesh (nerf_isosurface_grid, nerf_extract_mesh; conventions: include/nerf_mi355x.h, "isosurface meshes").
//
//   k_mesh_classify    one thread per lattice point A: which of the up to 7 edges A -> A + d, d in {0,1}^3 \ {0}, carry a vertex (both end
//                      sigma finite, exactly one end inside = sigma > iso), the inside mask of the 8 corners of the cell whose low corner A
//                      is, and that cell's triangle count (0 when a corner is missing or not finite).  k_mesh_classify_filtered: the same with
//                      "inside" = sigma > iso and the point's component kept (components_kernels.hip); every later kernel reads only the masks
//   k_mesh_block_sums  per block of 256 points the number of vertices and of triangles (wave ballots + 64-bit popcounts)
//   k_mesh_scan_sums   ONE workgroup: exclusive prefix sums of the block sums in place, 256 at a time with a carry; the totals
//   k_mesh_scan_add    per block the exclusive prefix sums of its points' counts + the block's offset -> vbase, tbase
//   k_mesh_vertices    one thread per lattice point: its vertices (position, normal, SoA copy, -normal) at vbase[A] + rank of the edge's bit
//   k_mesh_triangles   one thread per cell: the triangles of its six tetrahedra at tbase[A] ...; a vertex id is vbase of the owning lattice
//                      point + the rank of the edge's bit in that point's mask
// No kernel waits on another workgroup and no atomic is used: the kernel boundaries order the passes, the prefix sums fix every output
// position, so the mesh is the same bits in every run.  These are bookkeeping kernels bound by L2 / HBM traffic (8 neighbour loads per point,
// coalesced along x and served from cache); the corner sigma are not staged in LDS.
//
// The six tetrahedra of a cell with low corner c are (c, c + e_a, c + e_a + e_b, c + (1,1,1)) for the axis orders (a, b, .) = xyz, xzy, yxz,
// yzx, zxy, zyx: all share the body diagonal, their faces on a cell face use the diagonal through the face's low corner on both sides of
// the face, so neighbouring cells agree and the surface is watertight.  With corners as bit codes (x = 1, y = 2, z = 4) the four corners of a
// tetrahedron form a chain 0 < a < a|b < 7 of bit sets; an edge between corners i < j of the chain is owned by corner i and its bit is the
// set difference.  The tetrahedron (v0, v1, v2, v3) is positively oriented in index space iff (a, b, c) is an even permutation of (x, y, z).
//
// Winding (counter-clockwise seen from outside, in index space), derived rather than tabulated.  Write S = +1 / -1 for the orientation of
// (v0..v3) and det(p; q, r, s) = det[q - p, r - p, s - p] = S * sign of the permutation (p, q, r, s) of (0, 1, 2, 3).
//   one corner p inside, q < r < s outside: the triangle on the edges (pq, pr, ps) has its normal along det(p; q, r, s) * (away from p):
//     keep that order iff S * (-1)^p > 0 (moving p to the front of 0123 takes p transpositions), else swap the last two;
//   one corner p outside: the same with the sign reversed;
//   p1 < p2 inside, q1 < q2 outside: the quad's vertices in cyclic order are (p1q1, p1q2, p2q2, p2q1) (neighbours share a face of the
//     tetrahedron); that order has its normal towards the outside iff det(p1; p2, q1, q2) > 0, i.e. iff S * (-1)^inversions > 0 with
//     inversions = the number of pairs p_i > q_j; else the cycle is reversed.
// Canonical form: a triangle is rotated so that it starts with its smallest vertex id; a quad's cycle is rotated to start at its smallest id
// m and split along the diagonal through m into (m, q1, q2), (m, q2, q3).
//
// All vertex arithmetic is IEEE f32 with every operation rounded once (__f*_rn, which are the plain operators: the file is built with
// -ffp-contract=off like sampling_kernels.hip), division and square root correctly rounded (__fdiv_rn = `/`, sqrtf), and always runs from the owning point A to B, so every cell that shares an edge sees one vertex.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "isosurface_kernels.h"

namespace {

constexpr int kB = kMeshScanBlock;

__device__ __forceinline__ bool is_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ float lattice_coord(const MeshLattice &g, int k, int i) { return __fadd_rn(g.lo[k], __fmul_rn(g.step[k], (float)i)); }

// a + t * (b - a): subtract, multiply, add, each rounded once
__device__ __forceinline__ float lerp_rn(float a, float b, float t) { return __fadd_rn(a, __fmul_rn(t, __fsub_rn(b, a))); }

// mask of the four corners of the tetrahedron (0, a, a | b, 7) in an 8-bit corner mask
__host__ __device__ constexpr uint32_t tet_mask(int a, int b) { return 1u | (1u << a) | (1u << (a | b)) | (1u << 7); }

__device__ __forceinline__ uint32_t tet_triangle_count(uint32_t inm, uint32_t tm) {
    const int k = __popc(inm & tm);
    return k == 2 ? 2u : (k == 1 || k == 3) ? 1u : 0u;
}

// FILTER: a point of a discarded component counts as not inside -- the inside bit is ANDed with the keep flag (bit 31 of size[label], components_kernels.h)
// of the corner's component.  Without it this is the unfiltered classification, instruction for instruction.
template <bool FILTER>
__device__ __forceinline__ void classify_point(const float *__restrict__ sigma, const MeshLattice &g, uint32_t n, uint32_t *__restrict__ info,
                                               const uint32_t *__restrict__ label, const uint32_t *__restrict__ size) {
    const uint32_t A = blockIdx.x * (uint32_t)kB + threadIdx.x;
    if (A >= n) return;
    const uint32_t nx = (uint32_t)g.nx, ny = (uint32_t)g.ny, nz = (uint32_t)g.nz;
    const uint32_t ix = A % nx, row = A / nx, iy = row % ny, iz = row / ny;
    const bool hx = ix + 1 < nx, hy = iy + 1 < ny, hz = iz + 1 < nz;
    uint32_t fin = 0, inm = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const bool ok = (!(e & 1) || hx) && (!(e & 2) || hy) && (!(e & 4) || hz);
        if (ok) { // inside the lattice: A + offset < n
            const uint32_t P = A + (uint32_t)(e & 1) + nx * ((uint32_t)((e >> 1) & 1) + ny * (uint32_t)(e >> 2));
            const float s = sigma[P];
            fin |= (is_finite(s) ? 1u : 0u) << e;
            bool in = s > g.iso; // a NaN is not inside
            if (FILTER && in) {
                const uint32_t l = label[P]; // the root of an inside point: an index < n
                in = l < n && (size[l] >> 31) != 0u;
            }
            inm |= (in ? 1u : 0u) << e;
        }
    }
    uint32_t mask = 0;
    if (fin & 1u) {
        const uint32_t differs = (inm & 1u) ? ~inm : inm; // bit e: the other end's side differs from A's
        mask = fin & differs & 0xfeu;
    }
    uint32_t tri = 0;
    if (fin == 0xffu)
        tri = tet_triangle_count(inm, tet_mask(1, 2)) + tet_triangle_count(inm, tet_mask(1, 4)) + tet_triangle_count(inm, tet_mask(2, 1)) +
              tet_triangle_count(inm, tet_mask(2, 4)) + tet_triangle_count(inm, tet_mask(4, 1)) + tet_triangle_count(inm, tet_mask(4, 2));
    info[A] = mask | (inm << 8) | (tri << 16);
}

__global__ __launch_bounds__(kB) void k_mesh_classify(const float *__restrict__ sigma, MeshLattice g, uint32_t n, uint32_t *__restrict__ info) {
    classify_point<false>(sigma, g, n, info, nullptr, nullptr);
}

__global__ __launch_bounds__(kB) void k_mesh_classify_filtered(const float *__restrict__ sigma, MeshLattice g, uint32_t n, uint32_t *__restrict__ info,
                                                              const uint32_t *__restrict__ label, const uint32_t *__restrict__ size) {
    classify_point<true>(sigma, g, n, info, label, size);
}

// number of set bits over the wave of bit `bit` of v: one ballot, one 64-bit popcount
__device__ __forceinline__ uint32_t wave_count_bit(uint32_t v, int bit) { return (uint32_t)__popcll(__ballot((v >> bit) & 1u)); }

__global__ __launch_bounds__(kB) void k_mesh_block_sums(const uint32_t *__restrict__ info, uint32_t n, uint32_t *__restrict__ vsum, uint32_t *__restrict__ tsum) {
    __shared__ uint32_t s[kB / 64][2];
    const uint32_t A = blockIdx.x * (uint32_t)kB + threadIdx.x;
    const uint32_t w = A < n ? info[A] : 0u;
    uint32_t v = 0, t = 0;
#pragma unroll
    for (int e = 1; e < 8; ++e) v += wave_count_bit(w, e);
#pragma unroll
    for (int b = 0; b < 4; ++b) t += wave_count_bit(w, 16 + b) << b;
    if ((threadIdx.x & 63) == 0) { s[threadIdx.x >> 6][0] = v; s[threadIdx.x >> 6][1] = t; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kB / 64; ++k) { v += s[k][0]; t += s[k][1]; }
        vsum[blockIdx.x] = v; tsum[blockIdx.x] = t;
    }
}

__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

// exclusive prefix sums of (v, t) over the kB threads of the workgroup; sum_* = the workgroup's totals.  Ends with a barrier: s is free again.
__device__ __forceinline__ void block_exclusive2(uint32_t &v, uint32_t &t, uint32_t &sum_v, uint32_t &sum_t, uint32_t (*s)[2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t iv = wave_inclusive(v, lane), it = wave_inclusive(t, lane);
    if (lane == 63) { s[wave][0] = iv; s[wave][1] = it; }
    __syncthreads();
    uint32_t ov = 0, ot = 0;
    sum_v = 0; sum_t = 0;
#pragma unroll
    for (int k = 0; k < kB / 64; ++k) {
        if (k < wave) { ov += s[k][0]; ot += s[k][1]; }
        sum_v += s[k][0]; sum_t += s[k][1];
    }
    v = iv - v + ov; t = it - t + ot;
    __syncthreads();
}

__global__ __launch_bounds__(kB) void k_mesh_scan_sums(uint32_t *__restrict__ vsum, uint32_t *__restrict__ tsum, uint32_t n_blocks, uint32_t *__restrict__ totals) {
    __shared__ uint32_t s[kB / 64][2];
    uint32_t carry_v = 0, carry_t = 0;
    for (uint32_t base = 0; base < n_blocks; base += (uint32_t)kB) { // uniform trip count: every thread reaches the barriers
        const uint32_t i = base + threadIdx.x;
        uint32_t v = i < n_blocks ? vsum[i] : 0u, t = i < n_blocks ? tsum[i] : 0u, sv, stt;
        block_exclusive2(v, t, sv, stt, s);
        if (i < n_blocks) { vsum[i] = v + carry_v; tsum[i] = t + carry_t; }
        carry_v += sv; carry_t += stt;
    }
    if (threadIdx.x == 0) { totals[0] = carry_v; totals[1] = carry_t; }
}

__global__ __launch_bounds__(kB) void k_mesh_scan_add(const uint32_t *__restrict__ info, uint32_t n, const uint32_t *__restrict__ vsum,
                                                      const uint32_t *__restrict__ tsum, uint32_t *__restrict__ vbase, uint32_t *__restrict__ tbase) {
    __shared__ uint32_t s[kB / 64][2];
    const uint32_t A = blockIdx.x * (uint32_t)kB + threadIdx.x;
    const uint32_t w = A < n ? info[A] : 0u;
    uint32_t v = (uint32_t)__popc(w & 0xfeu), t = (w >> 16) & 15u, sv, stt;
    block_exclusive2(v, t, sv, stt, s);
    if (A < n) { vbase[A] = v + vsum[blockIdx.x]; tbase[A] = t + tsum[blockIdx.x]; }
}

// central difference of sigma over the central difference of the coordinate, indices clamped to the lattice (one-sided at the borders)
__device__ __forceinline__ void gradient_at(const float *__restrict__ sigma, const MeshLattice &g, uint32_t P, int ix, int iy, int iz, float (&out)[3]) {
    const int i[3] = {ix, iy, iz}, n[3] = {g.nx, g.ny, g.nz};
    const uint32_t stride[3] = {1u, (uint32_t)g.nx, (uint32_t)g.nx * (uint32_t)g.ny};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int im = max(i[k] - 1, 0), ip = min(i[k] + 1, n[k] - 1);
        const float sp = sigma[P + (uint32_t)(ip - i[k]) * stride[k]], sm = sigma[P - (uint32_t)(i[k] - im) * stride[k]];
        out[k] = __fdiv_rn(__fsub_rn(sp, sm), __fsub_rn(lattice_coord(g, k, ip), lattice_coord(g, k, im)));
    }
}

__global__ __launch_bounds__(kB) void k_mesh_vertices(const float *__restrict__ sigma, MeshLattice g, uint32_t n, const uint32_t *__restrict__ info,
                                                      const uint32_t *__restrict__ vbase, uint32_t n_vertices, float *__restrict__ vertices,
                                                      float *__restrict__ normals, float *__restrict__ pts_soa, float *__restrict__ neg_normals) {
    const uint32_t A = blockIdx.x * (uint32_t)kB + threadIdx.x;
    if (A >= n) return;
    const uint32_t mask = info[A] & 0xfeu;
    if (!mask) return;
    const uint32_t nx = (uint32_t)g.nx, ny = (uint32_t)g.ny;
    const int ix = (int)(A % nx), iy = (int)((A / nx) % ny), iz = (int)(A / nx / ny);
    const bool want_n = normals || neg_normals;
    const float sa = sigma[A];
    const float pa[3] = {lattice_coord(g, 0, ix), lattice_coord(g, 1, iy), lattice_coord(g, 2, iz)};
    float ga[3] = {0.f, 0.f, 0.f};
    if (want_n) gradient_at(sigma, g, A, ix, iy, iz, ga);
    uint32_t id = vbase[A];
    for (int e = 1; e < 8; ++e) {
        if (!((mask >> e) & 1u)) continue;
        if (id >= n_vertices) return; // cannot happen: the prefix sums come from the same masks
        const int dx = e & 1, dy = (e >> 1) & 1, dz = e >> 2; // the mask bit guarantees that B lies on the lattice
        const uint32_t B = A + (uint32_t)dx + nx * ((uint32_t)dy + ny * (uint32_t)dz);
        const float sb = sigma[B];
        const float t = __fdiv_rn(__fsub_rn(g.iso, sa), __fsub_rn(sb, sa));
        const float pb[3] = {dx ? lattice_coord(g, 0, ix + 1) : pa[0], dy ? lattice_coord(g, 1, iy + 1) : pa[1], dz ? lattice_coord(g, 2, iz + 1) : pa[2]};
        float p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = lerp_rn(pa[k], pb[k], t);
        if (vertices) { vertices[3 * (size_t)id] = p[0]; vertices[3 * (size_t)id + 1] = p[1]; vertices[3 * (size_t)id + 2] = p[2]; }
        if (pts_soa) { pts_soa[id] = p[0]; pts_soa[(size_t)n_vertices + id] = p[1]; pts_soa[2 * (size_t)n_vertices + id] = p[2]; }
        if (want_n) {
            float gb[3], gv[3], nrm[3];
            gradient_at(sigma, g, B, ix + dx, iy + dy, iz + dz, gb);
#pragma unroll
            for (int k = 0; k < 3; ++k) gv[k] = lerp_rn(ga[k], gb[k], t);
            // sqrtf, not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS the latter is the native (approximate) square root; sqrtf is correctly
            // rounded under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt, which sampling_kernels.hip relies on as well
            const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(gv[0], gv[0]), __fmul_rn(gv[1], gv[1])), __fmul_rn(gv[2], gv[2])));
            const bool ok = len != 0.0f && is_finite(len); // a NaN length is not finite
#pragma unroll
            for (int k = 0; k < 3; ++k) nrm[k] = ok ? __fdiv_rn(-gv[k], len) : 0.0f;
            if (normals) { normals[3 * (size_t)id] = nrm[0]; normals[3 * (size_t)id + 1] = nrm[1]; normals[3 * (size_t)id + 2] = nrm[2]; }
            if (neg_normals) { neg_normals[3 * (size_t)id] = -nrm[0]; neg_normals[3 * (size_t)id + 1] = -nrm[1]; neg_normals[3 * (size_t)id + 2] = -nrm[2]; }
        }
        ++id;
    }
}

// the ids of the six edges of a tetrahedron, in the order 01, 02, 03, 12, 13, 23; scalars and selects (no per-thread array: a runtime index would
// put it in scratch)
struct TetEdges { uint32_t e01, e02, e03, e12, e13, e23; };
__device__ __forceinline__ uint32_t pick6(const TetEdges E, int i) {
    const uint32_t a = E.e01, b = E.e02, c = E.e03, d = E.e12, e = E.e13, f = E.e23;
    return i == 0 ? a : i == 1 ? b : i == 2 ? c : i == 3 ? d : i == 4 ? e : f;
}

// the edge between corners i != j of the chain, as an index into TetEdges
__device__ __forceinline__ int pair_index(int i, int j) {
    const int lo = min(i, j), hi = max(i, j);
    return lo == 0 ? hi - 1 : lo + hi;
}

__device__ __forceinline__ void store_triangle(uint32_t *__restrict__ tris, uint32_t at, uint32_t n_triangles, uint32_t a, uint32_t b, uint32_t c) {
    if (at >= n_triangles) return; // cannot happen: the prefix sums come from the same counts
    tris[3 * (size_t)at] = a; tris[3 * (size_t)at + 1] = b; tris[3 * (size_t)at + 2] = c;
}

// the triangles of the tetrahedron (0, CA, CA | CB, 7) of one cell.  cb / cm: vbase and edge mask of the cell's 8 corners.
template <int CA, int CB>
__device__ __forceinline__ void tet_triangles(uint32_t inm, const uint32_t (&cb)[8], const uint32_t (&cm)[8], uint32_t *__restrict__ tris, uint32_t &at,
                                              uint32_t n_triangles) {
#define NERF_TET_CORNER(i) ((i) == 0 ? 0 : (i) == 1 ? CA : (i) == 2 ? (CA | CB) : 7) /* the chain 0 < a < a|b < 7 */
    constexpr bool even = (((CB >> 1) - (CA >> 1) + 3) % 3) == 1; // (a, b, c) an even permutation of (x, y, z): S = +1
    const uint32_t m = ((inm >> NERF_TET_CORNER(0)) & 1u) | (((inm >> NERF_TET_CORNER(1)) & 1u) << 1) | (((inm >> NERF_TET_CORNER(2)) & 1u) << 2) | (((inm >> NERF_TET_CORNER(3)) & 1u) << 3);
    const int k = __popc(m);
    if (k == 0 || k == 4) return;
    // vertex id of the edge between corners i < j: vbase of the owner + rank of the bit c[j] - c[i] in the owner's mask (valid only where the edge has a vertex)
#define NERF_EDGE_ID(i, j) (cb[NERF_TET_CORNER(i)] + (uint32_t)__popc(cm[NERF_TET_CORNER(i)] & ((1u << (NERF_TET_CORNER(j) - NERF_TET_CORNER(i))) - 1u)))
    const TetEdges E = {NERF_EDGE_ID(0, 1), NERF_EDGE_ID(0, 2), NERF_EDGE_ID(0, 3), NERF_EDGE_ID(1, 2), NERF_EDGE_ID(1, 3), NERF_EDGE_ID(2, 3)};
#undef NERF_EDGE_ID
#undef NERF_TET_CORNER
    if (k != 2) {
        const uint32_t lone = k == 1 ? m : (~m & 15u);
        const int p = __ffs(lone) - 1;
        const int o1 = p == 0 ? 1 : 0, o2 = p <= 1 ? 2 : 1, o3 = p == 3 ? 2 : 3;
        const uint32_t e1 = pick6(E, pair_index(p, o1)), e2 = pick6(E, pair_index(p, o2)), e3 = pick6(E, pair_index(p, o3));
        const bool keep = even != (((p & 1) != 0) != (k == 3)); // S * (-1)^p * (-1 if the lone corner is the outside one) > 0
        const uint32_t a = e1, b = keep ? e2 : e3, d = keep ? e3 : e2;
        // rotate so that the smallest id comes first
        if (a < b && a < d) store_triangle(tris, at, n_triangles, a, b, d);
        else if (b < d) store_triangle(tris, at, n_triangles, b, d, a);
        else store_triangle(tris, at, n_triangles, d, a, b);
        at += 1;
    } else {
        const uint32_t om = ~m & 15u;
        const int p1 = __ffs(m) - 1, p2 = 31 - __clz(m), q1 = __ffs(om) - 1, q2 = 31 - __clz(om);
        const int inversions = (p1 > q1) + (p1 > q2) + (p2 > q1) + (p2 > q2);
        const bool keep = even != ((inversions & 1) != 0);
        const uint32_t A0 = pick6(E, pair_index(p1, q1)), B0 = pick6(E, pair_index(p1, q2)), C0 = pick6(E, pair_index(p2, q2)), D0 = pick6(E, pair_index(p2, q1));
        const uint32_t y0 = A0, y1 = keep ? B0 : D0, y2 = C0, y3 = keep ? D0 : B0; // the cycle under the winding
        const uint32_t mn = min(min(y0, y1), min(y2, y3));
        const int r = mn == y0 ? 0 : mn == y1 ? 1 : mn == y2 ? 2 : 3;
        const uint32_t z1 = r == 0 ? y1 : r == 1 ? y2 : r == 2 ? y3 : y0;
        const uint32_t z2 = r == 0 ? y2 : r == 1 ? y3 : r == 2 ? y0 : y1;
        const uint32_t z3 = r == 0 ? y3 : r == 1 ? y0 : r == 2 ? y1 : y2;
        store_triangle(tris, at, n_triangles, mn, z1, z2);
        store_triangle(tris, at + 1, n_triangles, mn, z2, z3);
        at += 2;
    }
}

__global__ __launch_bounds__(kB) void k_mesh_triangles(MeshLattice g, uint32_t n, const uint32_t *__restrict__ info, const uint32_t *__restrict__ vbase,
                                                       const uint32_t *__restrict__ tbase, uint32_t n_triangles, uint32_t *__restrict__ tris) {
    const uint32_t A = blockIdx.x * (uint32_t)kB + threadIdx.x;
    if (A >= n) return;
    const uint32_t w = info[A];
    if (!((w >> 16) & 15u)) return; // no triangle; a count > 0 means that all 8 corners lie on the lattice (and are finite)
    const uint32_t nx = (uint32_t)g.nx, ny = (uint32_t)g.ny;
    uint32_t cb[8], cm[8];
#define NERF_LOAD_CORNER(e)                                                                                                  \
    {                                                                                                                        \
        const uint32_t P = A + (uint32_t)((e) & 1) + nx * ((uint32_t)(((e) >> 1) & 1) + ny * (uint32_t)((e) >> 2));          \
        cb[e] = vbase[P];                                                                                                    \
        cm[e] = info[P] & 0xfeu;                                                                                             \
    }
    NERF_LOAD_CORNER(0) NERF_LOAD_CORNER(1) NERF_LOAD_CORNER(2) NERF_LOAD_CORNER(3) NERF_LOAD_CORNER(4) NERF_LOAD_CORNER(5) NERF_LOAD_CORNER(6) NERF_LOAD_CORNER(7)
#undef NERF_LOAD_CORNER
    const uint32_t inm = (w >> 8) & 0xffu;
    uint32_t at = tbase[A];
    tet_triangles<1, 2>(inm, cb, cm, tris, at, n_triangles); // xyz
    tet_triangles<1, 4>(inm, cb, cm, tris, at, n_triangles); // xzy
    tet_triangles<2, 1>(inm, cb, cm, tris, at, n_triangles); // yxz
    tet_triangles<2, 4>(inm, cb, cm, tris, at, n_triangles); // yzx
    tet_triangles<4, 1>(inm, cb, cm, tris, at, n_triangles); // zxy
    tet_triangles<4, 2>(inm, cb, cm, tris, at, n_triangles); // zyx
}

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

} // namespace

size_t mesh_workspace_bytes(size_t n_points) {
    const size_t nb = (n_points + kB - 1) / kB;
    return 256 + 4 * round_up(n_points * 4, 256) + 2 * round_up(nb * 4, 256);
}

MeshWorkspace mesh_workspace_carve(void *base, size_t n_points) {
    MeshWorkspace w;
    const size_t nb = (n_points + kB - 1) / kB, per = round_up(n_points * 4, 256), per_b = round_up(nb * 4, 256);
    char *p = (char *)base;
    w.totals = (uint32_t *)p; p += 256;
    w.sigma = (float *)p; p += per;
    w.info = (uint32_t *)p; p += per;
    w.vbase = (uint32_t *)p; p += per;
    w.tbase = (uint32_t *)p; p += per;
    w.vsum = (uint32_t *)p; p += per_b;
    w.tsum = (uint32_t *)p;
    w.n_points = (uint32_t)n_points; w.n_blocks = (uint32_t)nb;
    return w;
}

hipError_t launch_mesh_count(const MeshLattice &g, const MeshWorkspace &w, hipStream_t st, const uint32_t *label, const uint32_t *size) {
    if (w.n_points == 0 || (size_t)g.nx * (size_t)g.ny * (size_t)g.nz != w.n_points || g.nx < 2 || g.ny < 2 || g.nz < 2 || (!label != !size)) return hipErrorInvalidValue;
    if (label) hipLaunchKernelGGL(k_mesh_classify_filtered, dim3(w.n_blocks), dim3(kB), 0, st, w.sigma, g, w.n_points, w.info, label, size);
    else hipLaunchKernelGGL(k_mesh_classify, dim3(w.n_blocks), dim3(kB), 0, st, w.sigma, g, w.n_points, w.info);
    hipLaunchKernelGGL(k_mesh_block_sums, dim3(w.n_blocks), dim3(kB), 0, st, w.info, w.n_points, w.vsum, w.tsum);
    hipLaunchKernelGGL(k_mesh_scan_sums, dim3(1), dim3(kB), 0, st, w.vsum, w.tsum, w.n_blocks, w.totals);
    return hipGetLastError();
}

hipError_t launch_mesh_emit(const MeshLattice &g, const MeshWorkspace &w, uint32_t n_vertices, float *vertices, float *normals, float *pts_soa,
                            float *neg_normals, uint32_t n_triangles, uint32_t *triangles, hipStream_t st) {
    if (w.n_points == 0 || (size_t)g.nx * (size_t)g.ny * (size_t)g.nz != w.n_points) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mesh_scan_add, dim3(w.n_blocks), dim3(kB), 0, st, w.info, w.n_points, w.vsum, w.tsum, w.vbase, w.tbase);
    if (n_vertices && (vertices || normals || pts_soa || neg_normals))
        hipLaunchKernelGGL(k_mesh_vertices, dim3(w.n_blocks), dim3(kB), 0, st, w.sigma, g, w.n_points, w.info, w.vbase, n_vertices, vertices, normals, pts_soa,
                           neg_normals);
    if (n_triangles && triangles)
        hipLaunchKernelGGL(k_mesh_triangles, dim3(w.n_blocks), dim3(kB), 0, st, g, w.n_points, w.info, w.vbase, w.tbase, n_triangles, triangles);
    return hipGetLastError();
}

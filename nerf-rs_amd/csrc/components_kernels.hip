// components_kernels.hip -- connected components of the inside points (sigma > iso) of a lattice under the 14-neighbour Kuhn connectivity, their
// sizes, their rank order and the keep flags of a filter (nerf_lattice_components, nerf_*_filtered; definition: include/nerf_mi355x.h, "lattice
// components").
//
//   k_cc_init       label[A] = 0xFFFFFFFF where A is not inside (sigma[A] > iso; a NaN is not inside, +inf is), else the first point of A's run of
//                   consecutive inside points along x within its wave and row (a ballot; A itself where the run starts there); size[A] = 0
//   k_cc_union      one thread per inside point A: unite A with the inside far ends of the up to 7 edges it owns (A + d, d in {0,1}^3 \ {0}).  Union-find
//                   on the label array itself: find both roots, link the larger root under the smaller with atomicMin; when the value the atomic
//                   returns shows that the node was no longer a root, carry on from the returned parent
//   k_cc_flatten    label[A] = root of A
//   k_cc_sizes      size[root] += 1 per point, aggregated over the wave first (one atomicAdd per distinct root of a wave); roots per block of 256
//   k_cc_scan_sums  ONE workgroup: exclusive prefix sums of the block sums, n_components; clears n_kept and the winners
//   k_cc_compact    the roots in ascending order (position = block offset + rank within the block)
//   k_cc_argmax     pass k of the ranking: the largest key (n_points << 32) | (0xFFFFFFFF - label) below the winner of pass k - 1, over the root
//                   list: wave maximum, then one 64-bit atomicMax per wave.  Keys are distinct, so K passes give the first K components in rank order
//   k_cc_keep       per root: kept iff n_points >= min_points and (keep_largest == 0 or key >= winner keep_largest - 1); the flag is bit 31 of
//                   size[root]; n_kept
//   k_cc_winners    the table's label and n_points from the winners' keys; root -> rank
//   k_cc_bounds     per point of a tabled component integer min / max of its index coordinates: LDS atomics per block, then one global atomic per
//                   touched table word
//
// Termination.  Labels only ever decrease (atomicMin, and the flatten pass stores a root, which is <= every label on the chain) and label[x] <= x
// holds from k_cc_init on, so every parent chain strictly descends: find ends after at most x steps, and every round of unite either returns or
// continues from a strictly smaller node.  The loops are lock-free retries: no thread waits for another workgroup -- there is no flag to spin
// on, no look-back and no grid barrier; the kernel boundaries order the passes.
// Determinism.  Linking always puts the larger root under the smaller, so whatever order the atomics land in, the root of a component is its
// smallest linear index: the labels are the same bits in every run.  Sizes and n_kept are integer sums, bounds integer minima / maxima, the
// winners maxima of distinct keys: all independent of the order of the atomics.  The root list is ordered by a scan, not by an atomic counter.
// Labels that other workgroups may be lowering are read through relaxed agent-scope atomic loads (a stale parent is still an ancestor, so a
// stale read costs a step, never correctness; being atomic, the load stays inside the retry loop).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "components_kernels.h"

namespace {

constexpr int kB = 256;
constexpr uint32_t kRootGridMax = 1024; // workgroups of the kernels that walk the root list (grid-stride)

__device__ __forceinline__ uint32_t load_label(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// x is an inside point.  p > x cannot happen (label[x] <= x); treating it like a root keeps the walk inside [0, x] whatever it reads.
__device__ __forceinline__ uint32_t find_root(const uint32_t *label, uint32_t x) {
    for (;;) {
        const uint32_t p = load_label(label + x);
        if (p >= x) return x;
        x = p;
    }
}

__device__ __forceinline__ void unite(uint32_t *label, uint32_t a, uint32_t b) {
    for (;;) {
        a = find_root(label, a); b = find_root(label, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(label + a, b); // a > b: the larger root goes under the smaller
        if (old == a) return;                         // a was a root and is linked now
        a = old; // a had a parent old < a already (label[a] is min(old, b) now): old's tree and b's still have to meet
    }
}

// Pre-merge: an inside point starts under the first point of its run of consecutive inside points along x
// within its wave and row (one ballot) instead of under itself.  That is a valid starting forest -- the parent is a smaller index of the same
// component -- so the result is the same; the union pass then starts from runs instead of points and its chains are shorter.

__global__ __launch_bounds__(kB) void k_cc_init(const float *__restrict__ sigma, float iso, uint32_t nx, uint32_t n, uint32_t *__restrict__ label,
                                                uint32_t *__restrict__ size) {
    const uint32_t A = blockIdx.x * (uint32_t)kB + threadIdx.x;
    const bool in = A < n && sigma[A] > iso; // a NaN is not inside; no early return: every lane takes part in the ballots
    uint32_t l = in ? A : kCompNone;
    const int lane = threadIdx.x & 63; // a workgroup starts at a multiple of 256: A - lane is the wave's first point
    const unsigned long long m = __ballot(in);
    const unsigned long long starts = __ballot(in && (lane == 0 || A % nx == 0u || !((m >> (lane - 1)) & 1ull))); // first of the wave, of a row, or after a gap
    if (in) l = A - (uint32_t)(lane - (63 - __clzll((long long)(starts & (~0ull >> (63 - lane)))))); // the nearest start at or below this lane: it exists
    if (A < n) { label[A] = l; size[A] = 0u; }
}

__global__ __launch_bounds__(kB) void k_cc_union(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t n, uint32_t *label) {
    const uint32_t A = blockIdx.x * (uint32_t)kB + threadIdx.x;
    if (A >= n) return;
    if (load_label(label + A) == kCompNone) return; // an inside point's label is an index, never this value
    const uint32_t ix = A % nx, row = A / nx, iy = row % ny, iz = row / ny;
    const bool hx = ix + 1 < nx, hy = iy + 1 < ny, hz = iz + 1 < nz;
#pragma unroll
    for (int e = 1; e < 8; ++e) {
        const bool ok = (!(e & 1) || hx) && (!(e & 2) || hy) && (!(e & 4) || hz);
        if (!ok) continue; // B = A + offset lies on the lattice: B < n
        const uint32_t B = A + (uint32_t)(e & 1) + nx * ((uint32_t)((e >> 1) & 1) + ny * (uint32_t)(e >> 2));
        if (load_label(label + B) != kCompNone) unite(label, A, B);
    }
}

__global__ __launch_bounds__(kB) void k_cc_flatten(uint32_t n, uint32_t *label) {
    const uint32_t A = blockIdx.x * (uint32_t)kB + threadIdx.x;
    if (A >= n) return;
    if (load_label(label + A) == kCompNone) return;
    __hip_atomic_store(label + A, find_root(label, A), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kB) void k_cc_sizes(const uint32_t *__restrict__ label, uint32_t n, uint32_t *__restrict__ size, uint32_t *__restrict__ bsum) {
    __shared__ uint32_t s[kB / 64];
    const uint32_t A = blockIdx.x * (uint32_t)kB + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const uint32_t r = A < n ? label[A] : kCompNone; // no early return: every lane takes part in the ballots
    unsigned long long active = __ballot(r != kCompNone);
    while (active) { // wave-uniform: one round per distinct root of the wave
        const int leader = __ffsll(active) - 1;
        const uint32_t lr = (uint32_t)__shfl((int)r, leader, 64);
        const unsigned long long m = __ballot(r == lr);
        if (lane == leader) atomicAdd(size + lr, (uint32_t)__popcll(m)); // lr is the label of an inside point: lr < n
        active &= ~m;
    }
    const uint32_t roots = (uint32_t)__popcll(__ballot(A < n && r == A));
    if (lane == 0) s[threadIdx.x >> 6] = roots;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int k = 0; k < kB / 64; ++k) t += s[k];
        bsum[blockIdx.x] = t;
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

// exclusive prefix sum of v over the kB threads of the workgroup; sum = the workgroup's total.  Ends with a barrier: s is free again.
__device__ __forceinline__ void block_exclusive(uint32_t &v, uint32_t &sum, uint32_t *s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t iv = wave_inclusive(v, lane);
    if (lane == 63) s[wave] = iv;
    __syncthreads();
    uint32_t ov = 0;
    sum = 0;
#pragma unroll
    for (int k = 0; k < kB / 64; ++k) {
        if (k < wave) ov += s[k];
        sum += s[k];
    }
    v = iv - v + ov;
    __syncthreads();
}

__global__ __launch_bounds__(kB) void k_cc_scan_sums(uint32_t *__restrict__ bsum, uint32_t n_blocks, uint32_t *__restrict__ counts, unsigned long long *__restrict__ win) {
    __shared__ uint32_t s[kB / 64];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += (uint32_t)kB) { // uniform trip count: every thread reaches the barriers
        const uint32_t i = base + threadIdx.x;
        uint32_t v = i < n_blocks ? bsum[i] : 0u, sum;
        block_exclusive(v, sum, s);
        if (i < n_blocks) bsum[i] = v + carry;
        carry += sum;
    }
    if (threadIdx.x == 0) { counts[0] = carry; counts[1] = 0u; }
    if (threadIdx.x < kCompMaxRank) win[threadIdx.x] = 0ull;
}

__global__ __launch_bounds__(kB) void k_cc_compact(const uint32_t *__restrict__ label, uint32_t n, const uint32_t *__restrict__ bsum, uint32_t *__restrict__ roots) {
    __shared__ uint32_t s[kB / 64];
    const uint32_t A = blockIdx.x * (uint32_t)kB + threadIdx.x;
    const bool root = A < n && label[A] == A;
    uint32_t v = root ? 1u : 0u, sum;
    block_exclusive(v, sum, s);
    const uint32_t at = v + bsum[blockIdx.x];
    if (root && at < n) roots[at] = A; // at < n_components <= n: the sums come from the same labels
}

__device__ __forceinline__ unsigned long long comp_key(uint32_t n_points, uint32_t label) { return ((unsigned long long)n_points << 32) | (unsigned long long)(kCompNone - label); }

__device__ __forceinline__ unsigned long long wave_max64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(kB) void k_cc_argmax(const uint32_t *__restrict__ roots, const uint32_t *__restrict__ size, const uint32_t *__restrict__ counts,
                                                  unsigned long long *win, uint32_t k) {
    const uint32_t n_roots = counts[0];
    const unsigned long long bound = k ? win[k - 1] : ~0ull; // written by the previous launch; 0: the components ran out
    unsigned long long best = 0ull;
    for (uint32_t i = blockIdx.x * (uint32_t)kB + threadIdx.x; i < n_roots; i += gridDim.x * (uint32_t)kB) {
        const uint32_t r = roots[i];
        const unsigned long long key = comp_key(size[r], r);
        if (key < bound && key > best) best = key;
    }
    best = wave_max64(best); // the lanes have left the loop: all of them take part
    if ((threadIdx.x & 63) == 0 && best) atomicMax(win + k, best);
}

__global__ __launch_bounds__(kB) void k_cc_keep(const uint32_t *__restrict__ roots, uint32_t *__restrict__ size, uint32_t *counts, const unsigned long long *__restrict__ win,
                                                uint32_t keep_largest, uint32_t min_points, uint32_t *__restrict__ rankmap) {
    const uint32_t n_roots = counts[0];
    const unsigned long long threshold = keep_largest ? win[keep_largest - 1] : 0ull; // 0: fewer components than keep_largest, every rank passes
    uint32_t kept = 0;
    for (uint32_t i = blockIdx.x * (uint32_t)kB + threadIdx.x; i < n_roots; i += gridDim.x * (uint32_t)kB) {
        const uint32_t r = roots[i], sz = size[r];
        if (sz >= min_points && comp_key(sz, r) >= threshold) { size[r] = sz | kCompKeepBit; ++kept; }
        if (rankmap) rankmap[r] = kCompNone;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) kept += __shfl_xor(kept, off, 64);
    if ((threadIdx.x & 63) == 0 && kept) atomicAdd(counts + 1, kept);
}

__global__ __launch_bounds__(kCompMaxRank) void k_cc_winners(const unsigned long long *__restrict__ win, uint32_t cap_table, int nx, int ny, int nz, uint32_t n,
                                                             CompEntry *__restrict__ table, uint32_t *__restrict__ rankmap) {
    const uint32_t k = threadIdx.x;
    if (k >= cap_table) return;
    const unsigned long long key = win[k];
    CompEntry e = {kCompNone, 0u, {nx, ny, nz, -1, -1, -1}};
    if (key) {
        e.label = kCompNone - (uint32_t)(key & 0xFFFFFFFFull);
        e.n_points = (uint32_t)(key >> 32);
        if (e.label < n) rankmap[e.label] = k;
    }
    table[k] = e;
}

__global__ __launch_bounds__(kB) void k_cc_bounds(const uint32_t *__restrict__ label, const uint32_t *__restrict__ rankmap, uint32_t n, int nx, int ny, int nz,
                                                  uint32_t cap_table, CompEntry *table) {
    __shared__ int b[kCompMaxRank][6];
    for (int i = threadIdx.x; i < kCompMaxRank * 6; i += kB) {
        const int j = i % 6;
        b[i / 6][j] = j == 0 ? nx : j == 1 ? ny : j == 2 ? nz : -1;
    }
    __syncthreads();
    const uint32_t A = blockIdx.x * (uint32_t)kB + threadIdx.x;
    const uint32_t l = A < n ? label[A] : kCompNone;
    if (l < n) { // a root
        const uint32_t k = rankmap[l];
        if (k < cap_table) { // cap_table <= kCompMaxRank
            const int ix = (int)(A % (uint32_t)nx), iy = (int)((A / (uint32_t)nx) % (uint32_t)ny), iz = (int)(A / (uint32_t)nx / (uint32_t)ny);
            atomicMin(&b[k][0], ix); atomicMin(&b[k][1], iy); atomicMin(&b[k][2], iz);
            atomicMax(&b[k][3], ix); atomicMax(&b[k][4], iy); atomicMax(&b[k][5], iz);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kCompMaxRank * 6; i += kB) {
        const int k = i / 6, j = i % 6, v = b[k][j];
        if ((uint32_t)k >= cap_table) continue;
        if (j < 3) { if (v != (j == 0 ? nx : j == 1 ? ny : nz)) atomicMin(&table[k].bounds[j], v); }
        else if (v != -1) atomicMax(&table[k].bounds[j], v);
    }
}

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

constexpr size_t kHeaderBytes = 4096, kWinAt = 256, kTableAt = 1024;
static_assert(kWinAt + kCompMaxRank * sizeof(unsigned long long) <= kTableAt && kTableAt + kCompMaxRank * sizeof(CompEntry) <= kHeaderBytes, "header layout");
static_assert(sizeof(CompEntry) == 32, "CompEntry mirrors nerf_component");

} // namespace

size_t comp_workspace_bytes(size_t n_points) {
    const size_t nb = (n_points + kB - 1) / kB;
    return kHeaderBytes + 2 * round_up(n_points * 4, 256) + round_up(nb * 4, 256);
}

CompWorkspace comp_workspace_carve(void *base, size_t n_points, uint32_t *roots, uint32_t *rankmap) {
    CompWorkspace w;
    const size_t nb = (n_points + kB - 1) / kB, per = round_up(n_points * 4, 256);
    char *p = (char *)base;
    w.counts = (uint32_t *)p;
    w.win = (unsigned long long *)(p + kWinAt);
    w.table = (CompEntry *)(p + kTableAt);
    p += kHeaderBytes;
    w.label = (uint32_t *)p; p += per;
    w.size = (uint32_t *)p; p += per;
    w.bsum = (uint32_t *)p;
    w.roots = roots; w.rankmap = rankmap;
    w.n_points = (uint32_t)n_points; w.n_blocks = (uint32_t)nb;
    return w;
}

hipError_t launch_components(const float *sigma, int nx, int ny, int nz, float iso, const CompWorkspace &w, uint32_t keep_largest, uint32_t min_points,
                             uint32_t cap_table, hipStream_t st) {
    if (w.n_points == 0 || nx < 1 || ny < 1 || nz < 1 || (size_t)nx * (size_t)ny * (size_t)nz != w.n_points || w.n_points > (1u << 28) ||
        keep_largest > (uint32_t)kCompMaxRank || cap_table > (uint32_t)kCompMaxRank || !sigma || !w.roots || (cap_table && !w.rankmap))
        return hipErrorInvalidValue;
    const uint32_t n = w.n_points;
    const dim3 grid(w.n_blocks), block(kB), root_grid(w.n_blocks < kRootGridMax ? w.n_blocks : kRootGridMax);
    hipLaunchKernelGGL(k_cc_init, grid, block, 0, st, sigma, iso, (uint32_t)nx, n, w.label, w.size);
    hipLaunchKernelGGL(k_cc_union, grid, block, 0, st, (uint32_t)nx, (uint32_t)ny, (uint32_t)nz, n, w.label);
    hipLaunchKernelGGL(k_cc_flatten, grid, block, 0, st, n, w.label);
    hipLaunchKernelGGL(k_cc_sizes, grid, block, 0, st, w.label, n, w.size, w.bsum);
    hipLaunchKernelGGL(k_cc_scan_sums, dim3(1), block, 0, st, w.bsum, w.n_blocks, w.counts, w.win);
    hipLaunchKernelGGL(k_cc_compact, grid, block, 0, st, w.label, n, w.bsum, w.roots);
    const uint32_t passes = keep_largest > cap_table ? keep_largest : cap_table;
    for (uint32_t k = 0; k < passes; ++k) hipLaunchKernelGGL(k_cc_argmax, root_grid, block, 0, st, w.roots, w.size, w.counts, w.win, k);
    hipLaunchKernelGGL(k_cc_keep, root_grid, block, 0, st, w.roots, w.size, w.counts, w.win, keep_largest, min_points, cap_table ? w.rankmap : nullptr);
    if (cap_table) {
        hipLaunchKernelGGL(k_cc_winners, dim3(1), dim3(kCompMaxRank), 0, st, w.win, cap_table, nx, ny, nz, n, w.table, w.rankmap);
        hipLaunchKernelGGL(k_cc_bounds, grid, block, 0, st, w.label, w.rankmap, n, nx, ny, nz, cap_table, w.table);
    }
    return hipGetLastError();
}

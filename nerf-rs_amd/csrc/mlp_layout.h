// mlp_layout.h -- shared (host packer + device kernel) description of the packed weight stream.
//
// The fused MLP kernel (mlp_kernel.hip) keeps a wave's activations in registers in the C/D layout
// of v_mfma_f32_32x32x2_f32: a wave owns 32 points; lane l = (p = l & 31, h = l >> 5); an activation
// "tile" is 16 registers, register r of tile t on lane (p,h) holds feature
//       F(t, r, h) = 32 t + (r & 3) + 8 (r >> 2) + 4 h            of point p.
// One MFMA k-step (K = 2) takes register r of input tile t as its B operand (B[k = h][j = p]), so
// the two k-rows of step s = 16 t + r are features F(t,r,0) and F(t,r,1).  The A operand of the MFMA
// for output tile nt is therefore  A[i = l & 31][k = l >> 5] = W[row(s, h)][32 nt + i].
//
// Weight stream: for each layer, for each k-step s, for each group g of 4 output tiles, one 1-KiB
// "piece":   piece[(l * 4 + q)] = W[row(s, l >> 5)][32 (4 g + q) + (l & 31)]      (l = lane 0..63)
// so a wave fetches its A operands for 4 MFMAs with one conflict-free ds_read_b128.  The stream is
// cut in 16-KiB chunks (= 64/NT k-steps) which the kernel DMA's into a 3-slot LDS ring in order.
#pragma once
#include <stdint.h>

namespace nerfmlp {

constexpr int kChunkBytes = 16384;
constexpr int kChunkFloats = kChunkBytes / 4;
#ifndef NERF_RING_SLOTS
#define NERF_RING_SLOTS 3
#endif
constexpr int kRingSlots = NERF_RING_SLOTS; // >= 3; chunk c + kRingSlots - 1 is DMA'd while chunk c is consumed
constexpr int kPointsPerWave = 32;
constexpr int kWavesPerBlock = 4;
constexpr int kPointsPerBlock = kPointsPerWave * kWavesPerBlock;

// ---- ray grouping (f32 kernels, MLP_MODE_RAYS): which 32 consecutive sample slots a wave of a workgroup tile evaluates.
// Ungrouped, wave w of workgroup tile T takes wave tile 4 T + w (slots 128 T + 32 w ...): 128 consecutive samples, most of one ray.  The
// four waves meet at a barrier per weight chunk, so with zero-step skipping a chunk lasts as long as the wave with the fewest dead
// k-steps -- and the wave at the surface has fewer than the three in empty space, for the whole tile.  Grouped, the four
// waves take the SAME segment of four neighbouring rays, which are alike: with S = samples_per_ray / 32 segments per ray, rays go in
// blocks of four, and wave w of workgroup tile T = b S + j (j < S) takes segment j of ray 4 b + w = wave tile 4 b S + w S + j.  The
// last n_rays % 4 rays (workgroup tiles >= group_tiles) keep the ungrouped mapping.  A permutation of the wave tiles: every point is
// evaluated alone, so no value changes.  The kernel and nerf_debug_ray_grouping (the tests) call the same two functions.
#if defined(__HIPCC__) || defined(__CUDACC__)
#define NERF_HOST_DEVICE __host__ __device__
#else
#define NERF_HOST_DEVICE
#endif
struct RayGrouping {
    int segments;    // S; 0 = grouping off
    int group_tiles; // (n_rays / 4) * S workgroup tiles are grouped
};
// on iff allowed, whole 32-sample segments per ray, and at least one block of four rays (S = 1 gives the ungrouped mapping again)
NERF_HOST_DEVICE inline RayGrouping ray_grouping_of(int n_points, int samples_per_ray, bool allowed) {
    RayGrouping g = {0, 0};
    if (!allowed || samples_per_ray <= 0 || samples_per_ray % kPointsPerWave != 0 || n_points <= 0) return g;
    const int n_rays = n_points / samples_per_ray;
    if (n_rays < kWavesPerBlock) return g;
    g.segments = samples_per_ray / kPointsPerWave;
    g.group_tiles = (n_rays / kWavesPerBlock) * g.segments;
    return g;
}
// first sample slot of wave `wave` of workgroup tile `tile` (one wave-uniform division per call)
NERF_HOST_DEVICE inline int ray_group_first_slot(int tile, int wave, int segments, int group_tiles) {
    int wave_tile = tile * kWavesPerBlock + wave;
    if (segments > 0 && tile < group_tiles) {
        const int b = (int)((unsigned)tile / (unsigned)segments), j = tile - b * segments;
        wave_tile = (b * kWavesPerBlock + wave) * segments + j;
    }
    return wave_tile * kPointsPerWave;
}

// ---- wave tiling (f32 kernels, MLP_MODE_RAYS, image passes): which 32 samples make up a wave tile.  Untiled, a wave holds 32 consecutive
// samples of one ray -- in the coarse pass half of near..far, over which few hidden units are dead on all 32 columns.  A zero k-step needs one
// B register = two hidden units dead on ALL of the wave's points (mlp_f32_core.hip.h tile_steps), and neighbouring pixels' rays at the same
// sample index lie far closer together than 32 samples of one ray do.  Tiled, a wave holds ss consecutive samples of each ray of a tw x th
// block of pixels (tw th ss = 32).  An image pass is R whole rows of rw rays, spr samples each (slot = ray * spr + sample):
//   bundle   = a tw x th block of pixels, numbered row-major over the (rw / tw) x (R / th) grid;
//   wave tile (bundle, j), j < S_t = spr / ss, holds samples j ss .. j ss + ss - 1 of the bundle's tw th rays; lane p = (dy, dx, ds) with
//              ds = p % ss, dx = (p / ss) % tw, dy = p / (ss tw):
//              slot = ((by th + dy) rw + bx tw + dx) spr + j ss + ds = [wave-uniform base of the wave tile] + [lane part (dy rw + dx) spr + ds];
//   workgroup tiles of the tiled region come from ray_group_first_slot with bundle for ray and S_t for S (grouped: wave w of tile b S_t + j takes
//              wave tile j of bundle 4 b + w; ungrouped: four consecutive wave tiles).  S_t is a multiple of 4: whole 128-point tiles, no padding;
//   tail     = the last R % th rows, contiguous slots behind the tiled region, keep the untiled mapping (ray grouping of those rows), shifted.
// Again a permutation of the launch's points, every one evaluated alone in its MFMA column: no value changes.  Outputs go to sigma_out[slot] /
// rgb_out[3 slot] as before: a cache line of them is now written in parts by several workgroups, which needs no synchronisation -- every byte
// has exactly one writer, and nothing reads the arrays before the launch ends.
struct WaveTiling {
    int ss;            // consecutive samples per ray in a wave; 0 = tiling off (the other fields are then unused)
    int tw, th;        // pixels per bundle
    int rw, spr;       // rays per row, samples per ray
    int bundles_x;     // rw / tw
    int segments;      // S_t of a grouped launch, 0 = four consecutive wave tiles per workgroup tile
    int group_tiles;   // workgroup tiles [0, group_tiles) of the tiled region are grouped
    int tiled_tiles;   // workgroup tiles [0, tiled_tiles) are tiled ...
    int tiled_points;  // ... and cover slots [0, tiled_points); the tail's slots follow
};
// Pixel block a pass kind starts from (tw is halved until it divides rw).  These are the CPU model's best shape per pass (tools/wave_tile_model.py,
// profiles/wavetile_cpu_model.txt), and each beats the untiled kernel on the device by far more than the launch spread.  They are the
// only shapes measured on the device so far: the model's other candidates (8x1x4, 4x4x2; 8x4x1 for the full launch) are still to be A/B'd there.
constexpr int kWaveTileSigmaW = 8, kWaveTileSigmaH = 4; // sigma-only sampling launch: 8 x 4 pixels x 1 sample
constexpr int kWaveTileFullW = 4, kWaveTileFullH = 2;   // full launch: 4 x 2 pixels x 4 samples
// on iff allowed, whole 32-sample segments per ray, an image pass (rw > 0 rays per row, whole rows) of at least th rows, and a block of at least 4 pixels
NERF_HOST_DEVICE inline WaveTiling wave_tiling_of(int n_points, int samples_per_ray, int rw, bool full, bool allowed, bool grouping) {
    WaveTiling w = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!allowed || rw <= 0 || samples_per_ray <= 0 || samples_per_ray % kPointsPerWave != 0 || n_points <= 0) return w;
    const int n_rays = n_points / samples_per_ray;
    if (n_rays % rw != 0 || n_rays * samples_per_ray != n_points) return w;
    int tw = full ? kWaveTileFullW : kWaveTileSigmaW;
    const int th = full ? kWaveTileFullH : kWaveTileSigmaH;
    if (tw <= 0 || th <= 0) return w;
    while (rw % tw != 0) tw >>= 1;
    const int rows = n_rays / rw;
    if (rows < th || tw * th < 4 || kPointsPerWave % (tw * th) != 0) return w;
    w.ss = kPointsPerWave / (tw * th);
    w.tw = tw; w.th = th; w.rw = rw; w.spr = samples_per_ray;
    w.bundles_x = rw / tw;
    const int s_t = samples_per_ray / w.ss, n_bundles = w.bundles_x * (rows / th);
    w.tiled_points = (rows / th) * th * rw * samples_per_ray;
    w.tiled_tiles = w.tiled_points / kPointsPerBlock;
    if (grouping && n_bundles >= kWavesPerBlock) { w.segments = s_t; w.group_tiles = (n_bundles / kWavesPerBlock) * s_t; }
    return w;
}
// lane p's part of a tiled slot
NERF_HOST_DEVICE inline int wave_tile_lane_part(const WaveTiling &w, int p) {
    const int ds = p % w.ss, q = p / w.ss;
    return ((q / w.tw) * w.rw + q % w.tw) * w.spr + ds;
}
// the wave-uniform part of wave `wave` of workgroup tile `tile` < tiled_tiles (two wave-uniform divisions more than ray_group_first_slot)
NERF_HOST_DEVICE inline int wave_tile_base_slot(const WaveTiling &w, int tile, int wave) {
    const int s_t = w.spr / w.ss;
    const int wave_tile = ray_group_first_slot(tile, wave, w.segments, w.group_tiles) / kPointsPerWave;
    const int bundle = (int)((unsigned)wave_tile / (unsigned)s_t), j = wave_tile - bundle * s_t;
    const int by = (int)((unsigned)bundle / (unsigned)w.bundles_x), bx = bundle - by * w.bundles_x;
    return (by * w.th * w.rw + bx * w.tw) * w.spr + j * w.ss;
}
// One ray-mode launch's whole mapping: tiled region + tail (the ray grouping of the tail's rays; with tiling off, of the whole launch)
struct RayLaunchMap {
    WaveTiling wt;
    RayGrouping tail;
};
NERF_HOST_DEVICE inline RayLaunchMap ray_launch_map_of(int n_points, int samples_per_ray, int rw, bool full, bool grouping, bool tiling) {
    RayLaunchMap m;
    m.wt = wave_tiling_of(n_points, samples_per_ray, rw, full, tiling, grouping);
    m.tail = ray_grouping_of(n_points - (m.wt.ss ? m.wt.tiled_points : 0), samples_per_ray, grouping);
    return m;
}
// slot of lane p (0..31) of wave `wave` of workgroup tile `tile`; lane_part = wave_tile_lane_part(m.wt, p) (anything if tiling is off).
// May lie at or beyond n_points in the launch's last tile and in the look-ahead tile: the caller clamps / masks as before.
// The kernel forms the wave-uniform part once per tile (ray_launch_base) and adds the lane's part (tiled: lane_part, else p).
NERF_HOST_DEVICE inline bool ray_launch_tiled(const RayLaunchMap &m, int tile) { return m.wt.ss != 0 && tile < m.wt.tiled_tiles; }
NERF_HOST_DEVICE inline int ray_launch_base(const RayLaunchMap &m, int tile, int wave) {
    if (ray_launch_tiled(m, tile)) return wave_tile_base_slot(m.wt, tile, wave);
    const int first = m.wt.ss ? m.wt.tiled_tiles : 0, shift = m.wt.ss ? m.wt.tiled_points : 0;
    return shift + ray_group_first_slot(tile - first, wave, m.tail.segments, m.tail.group_tiles);
}
NERF_HOST_DEVICE inline int ray_launch_slot(const RayLaunchMap &m, int tile, int wave, int p, int lane_part) {
    return ray_launch_base(m, tile, wave) + (ray_launch_tiled(m, tile) ? lane_part : p);
}

// ---- depth ordering (f32 kernels, the full ray-mode launch of an image pass): wave tiles cut from the depth-sorted samples of a pixel block.
// The fine pass places each ray's importance samples differently, so "sample index k" is another depth on every ray of a static tile and the
// wave's 32 points are spread along the rays.  Ordered, the spr samples of all 32 rays of an 8 x 4 pixel block are merged by depth t (a device
// table, sampling_kernels.hip k_depth_order: position q of block b's sorted order holds the slot ray * spr + sample), and the block's
// 32 spr points are cut into waves of 32 in that order: workgroup tile T takes table entries 128 T .. 128 T + 127, four consecutive depth slabs
// of one block (tools/depth_order_model.py: the best of the compositions modelled).  Blocks are numbered row-major over the (rw / 8) x (rows / 4)
// grid; the region covers the first (rows / 4) * 4 rows = slots [0, points) = workgroup tiles [0, tiles), whole (32 spr is a multiple of 128).
// The rows behind it are a launch of their own shape (ray_launch_map_of of the remaining points), shifted by `points` slots and `tiles` tiles.
// A permutation of the launch's points as the two mappings above, if the table is a permutation of each block's slots -- the order kernel
// sorts (key, slot) pairs, so it is one for any bits of t.  Not for skip_empty launches: their workgroup vote spans the 128 points of a tile.
constexpr int kDepthBlockW = 8, kDepthBlockH = 4;
constexpr int kDepthOrderMaxSpr = 512; // the order kernel sorts a block's 32 spr keys (padded to a power of two) in LDS: 8 bytes each
struct DepthOrder {
    int tiles;     // workgroup tiles [0, tiles) are ordered; 0 = off
    int points;    // ... and cover slots [0, points)
    int blocks_x;  // rw / 8
    int blocks;    // pixel blocks of the region
};
NERF_HOST_DEVICE inline DepthOrder depth_order_of(int n_points, int samples_per_ray, int rw, bool full, bool allowed) {
    DepthOrder d = {0, 0, 0, 0};
    if (!allowed || !full || rw <= 0 || rw % kDepthBlockW != 0 || samples_per_ray <= 0 || samples_per_ray % kPointsPerWave != 0 ||
        samples_per_ray > kDepthOrderMaxSpr || n_points <= 0) return d;
    const int n_rays = n_points / samples_per_ray;
    if (n_rays % rw != 0 || n_rays * samples_per_ray != n_points) return d;
    const int rows = n_rays / rw;
    if (rows < kDepthBlockH) return d;
    d.blocks_x = rw / kDepthBlockW;
    d.blocks = d.blocks_x * (rows / kDepthBlockH);
    d.points = (rows / kDepthBlockH) * kDepthBlockH * rw * samples_per_ray;
    d.tiles = d.points / kPointsPerBlock;
    return d;
}
// slot of sample s of ray (dy, dx) of pixel block b: what the order kernel stores for it
NERF_HOST_DEVICE inline int depth_block_slot(int b, int blocks_x, int rw, int spr, int ray_in_block, int s) {
    const int by = (int)((unsigned)b / (unsigned)blocks_x), bx = b - by * blocks_x;
    const int dy = ray_in_block / kDepthBlockW, dx = ray_in_block % kDepthBlockW;
    return ((by * kDepthBlockH + dy) * rw + bx * kDepthBlockW + dx) * spr + s;
}

// ---- tile rotation (f32 fused kernel): in round k persistent workgroup c of G takes tile k G + ((c + k) mod G), not k G + c.  A launch's
// tiles come in periods (64 sample indices of the coarse pass, the depth slabs of a block in an ordered fine pass) whose cost differs
// systematically, and 256 is a multiple of those periods: unrotated, a workgroup sees the same class in every round and the slowest class
// sets the launch time.  Every tile below n_tiles is still taken exactly once (a round is a permutation of its G tiles).
NERF_HOST_DEVICE inline int rotated_tile(int k, int c, int G) {
    const int r = (int)((unsigned)(c + k % G) % (unsigned)G);
    return k * G + r;
}
// The same sequence without a division, as the kernel walks it: start at round 0 (tile c), tile_walk_next gives round 1's tile, round 2's, ...
// With rotate == false: k G + c.  nerf_debug_tile_rotation (tests/test_tile_rotation_host.py) walks it for every workgroup and compares it
// with rotated_tile.
struct TileWalk {
    int round_base, rot; // k G and k mod G of the round whose tile was formed last
};
NERF_HOST_DEVICE inline int tile_walk_next(TileWalk &w, int c, int G, bool rotate) {
    w.round_base += G;
    if (rotate) w.rot = w.rot + 1 == G ? 0 : w.rot + 1;
    const int r = c + w.rot;
    return w.round_base + (r >= G ? r - G : r);
}

// ---- coarse cut (f32 sigma-only ray-mode launch whose densities only the resampler reads): the resampler gives every sample behind the
// reference's T < 1e-4 cut the weight 0 whatever its sigma (sampling_kernels.hip weights_scan; src/lib.rs:273-279), so a workgroup that walks
// a pixel block's samples front to back may stop once all 32 rays of the block are cut.  The launch's tiled region then takes the UNGROUPED
// 8 x 4 x 1 map (ray_cut_map_of): wave w of tile k of block b holds sample index 4 k + w of the block's 32 rays, a block is spr / 4 consecutive
// workgroup tiles, and a lane keeps its ray for the whole block.  The persistent workgroups take UNITS, not tiles: unit u < blocks is pixel
// block u (tiles u spr/4 ..., walked in order until the block is cut), every unit behind them one tile of the untiled remainder (tail rows).
// Workgroup c of G starts with units c and G + c; further units come from a device-side counter (mlp_kernel.hip).  The kernel and
// nerf_debug_coarse_cut_walk (tests/test_coarse_cut_host.py) call the same functions.
struct RayCutWalk {
    int blocks;      // units [0, blocks) are pixel blocks; 0 = the launch does not qualify (the other fields are then 0)
    int block_tiles; // workgroup tiles per block: spr / 4
    int rest_first;  // units [blocks, blocks + rest_tiles) are the single tiles rest_first, rest_first + 1, ... (= blocks * block_tiles)
    int rest_tiles;
};
// the map of a cut launch: m with the tiled region ungrouped; the tail keeps its grouping
NERF_HOST_DEVICE inline RayLaunchMap ray_cut_map_of(RayLaunchMap m) {
    m.wt.segments = 0; m.wt.group_tiles = 0;
    return m;
}
// qualifies iff the sampling launch's 8 x 4 pixels x 1 sample tiling applies (whole 128-point tiles: spr a multiple of 4 follows from the tiling's 32)
NERF_HOST_DEVICE inline RayCutWalk ray_cut_walk_of(const RayLaunchMap &m, int n_points) {
    RayCutWalk w = {0, 0, 0, 0};
    if (m.wt.ss != 1 || m.wt.tw != kWaveTileSigmaW || m.wt.th != kWaveTileSigmaH || m.wt.segments != 0 || m.wt.spr % kWavesPerBlock != 0 || m.wt.tiled_tiles <= 0) return w;
    w.block_tiles = m.wt.spr / kWavesPerBlock;
    w.blocks = m.wt.tiled_tiles / w.block_tiles;
    w.rest_first = m.wt.tiled_tiles;
    w.rest_tiles = (n_points + kPointsPerBlock - 1) / kPointsPerBlock - m.wt.tiled_tiles;
    return w;
}
NERF_HOST_DEVICE inline int ray_cut_units(const RayCutWalk &w) { return w.blocks + w.rest_tiles; }
// first tile of unit u >= 0; n_tiles (no tile) for a unit beyond the launch's
NERF_HOST_DEVICE inline int ray_cut_unit_tile(const RayCutWalk &w, int u, int n_tiles) {
    if (u < w.blocks) return u * w.block_tiles;
    return u - w.blocks < w.rest_tiles ? w.rest_first + (u - w.blocks) : n_tiles;
}
// tile `tile` of unit u is done, all_cut: every ray of its block is cut behind it -> the unit's next tile, or -1: the unit is finished
NERF_HOST_DEVICE inline int ray_cut_next_in_unit(const RayCutWalk &w, int u, int tile, bool all_cut) {
    if (u >= w.blocks || all_cut) return -1;
    return tile + 1 < (u + 1) * w.block_tiles ? tile + 1 : -1;
}
constexpr int kCutLdsBytes = (kPointsPerBlock + 4) * 4; // behind the kernel's LDS: the tile's 128 alphas, and the unit handed out last

// ---- fine cut (f32 full ray-mode launch of a plain image render, depth-ordered; its sigma and rgb go to the compositor alone): k_composite
// freezes T and gives every later sample the weight 0 once a ray's T < 1e-4 (sampling_kernels.hip; src/lib.rs:273-279), so a workgroup that
// walks a pixel block's ORDERED tiles front to back may leave the block once all 32 rays are cut.  The same unit walk as the coarse cut's:
// unit u < DepthOrder.blocks is pixel block u = the spr / 4 consecutive tiles of its part of the order table, every tile of the static
// remainder behind order_tiles a unit of its own.  A lane changes its ray from tile to tile here, so the tile's alphas are posted by (ray in
// block, sample index) to LDS and lane r of every wave walks ray r's samples in index order.  That needs a ray's samples to stand in the
// table in index order, which holds exactly when the keys of every row of the block ascend: k_depth_order leaves one word per block
// (1: they do) and a block whose word is 0 is walked to its end.  The kernel and nerf_debug_fine_cut_walk (tests/test_fine_cut_host.py)
// call the same functions.
NERF_HOST_DEVICE inline RayCutWalk fine_cut_walk_of(int order_tiles, int samples_per_ray, int n_points) { // order_tiles: DepthOrder.tiles
    RayCutWalk w = {0, 0, 0, 0};
    if (order_tiles <= 0 || samples_per_ray <= 0 || samples_per_ray % kPointsPerWave != 0) return w;
    w.block_tiles = samples_per_ray / kWavesPerBlock; // 32 spr points / 128
    w.blocks = order_tiles / w.block_tiles;           // DepthOrder.blocks
    w.rest_first = order_tiles;
    w.rest_tiles = (n_points + kPointsPerBlock - 1) / kPointsPerBlock - order_tiles;
    return w;
}
// Behind the kernel's LDS in a fine-cut launch: the alphas of the tile by (ray in block, sample index mod 128) -- a ray has at most 128 samples
// in a tile, and those are consecutive indices; rows padded to 129 words so that 32 rays at the same index read 32 banks --, each ray's number
// of samples in the tile (two sets, taken in turn), and the unit handed out last.
constexpr int kFineCutRowWords = kPointsPerBlock + 1;
constexpr int kFineCutCountOff = 32 * kFineCutRowWords;      // words
constexpr int kFineCutUnitOff = kFineCutCountOff + 2 * 32;
constexpr int kFineCutLdsBytes = (kFineCutUnitOff + 4) * 4;  // 16 784

// k-steps per layer (K padded to the 32-slot tiles) and output tiles
constexpr int kStepsL0 = 32;    // 64 encoding slots (63 used)
constexpr int kStepsHid = 128;  // 256
constexpr int kStepsL5 = 160;   // 64 encoding slots + 256
constexpr int kStepsView = 144; // 256 + 32 dir slots (27 used)

constexpr int chunksOf(int steps, int nt) { return steps * nt * 256 / kChunkBytes; }

// layer order in the stream: dense0..dense7, [sigma-only kernels stop here], bottleneck, viewdirs
constexpr int kChunksSigma = chunksOf(kStepsL0, 8) + 4 * chunksOf(kStepsHid, 8) + chunksOf(kStepsL5, 8) +
                             2 * chunksOf(kStepsHid, 8);                                  // 120
constexpr int kChunksFull = kChunksSigma + chunksOf(kStepsHid, 8) + chunksOf(kStepsView, 4); // 145

// The f32 kernels read a FOLDED image of that stream (host_util.cpp fold_network): the bottleneck has no activation and the
// viewdirs layer is its only consumer, so W' = W_b . W_v[0:256] (256 x 128) and b' = b_v + b_b^T . W_v[0:256] replace the two
// layers.  Stream: the sigma part unchanged, W' as a 4-output-tile layer over relu(h7) (rows permuted like the bottleneck's),
// the dir-encoding chunk of viewdirs unchanged.  Small block: b' in the viewdirs bias slot, the rest unchanged.
constexpr int kStepsViewFolded = kStepsHid + 16;                                         // 256 + 32 dir slots: the same 144 k-steps
constexpr int kChunksColourFolded = chunksOf(kStepsViewFolded, 4);                       // 8 (W') + 1 (dir encoding) = 9
constexpr int kChunksFullFolded = kChunksSigma + kChunksColourFolded;                    // 129
constexpr int kFoldDirChunk = kChunksFull - 1;                                           // chunk of the packed stream that moves to the end of the folded one

// small parameters kept resident in LDS (floats)
constexpr int kBiasOff = 0;                     // 9 layers x [8 nt][2 h][16]  (dense0..7, bottleneck)
constexpr int kBiasViewOff = kBiasOff + 9 * 256; // [4 nt][2 h][16]
constexpr int kAlphaWOff = kBiasViewOff + 128;  // [2 h][128]
constexpr int kRgbWOff = kAlphaWOff + 256;      // [2 h][3 c][64]
constexpr int kMiscOff = kRgbWOff + 384;        // alpha bias, rgb bias r,g,b
constexpr int kSmallFloats = ((kMiscOff + 4 + 63) / 64) * 64; // 3136
constexpr int kSmallBytes = kSmallFloats * 4;

constexpr int kLdsBytes = kRingSlots * kChunkBytes + kSmallBytes;

// ---- 16-bit pieces (what the four 16-bit streams below are made of; host_util.cpp build_streams): a layer's weights in 1-KiB pieces of
// 64 lanes x 8 elements, one per k-step ks of K = 16 (two per 32-row input tile: ks >> 1 is the tile, ks & 1 its half) and output tile nt:
//       piece(ks, nt)[l * 8 + j] = W[row(ks >> 1, 8 (ks & 1) + j, l >> 5)][32 nt + (l & 31)]
// where row(tile, r, h) is the weight row that register r of input tile `tile` holds on lane-half h (regFeature / posSlotFeature /
// dirSlotFeature below; 0 for a padding slot): element j of the MFMA's B fragment.  K-steps per layer: dense0 4, hidden 16, dense5 20, viewdirs 18.
constexpr int kPieces16 = 8 * (4 + 4 * 16 + 20 + 3 * 16) + 4 * 18;  // 1160 pieces per network

// ---- bf16 stream v2 (mlp_kernel_bf16v2.hip): output-tile-major.  Per layer, per output tile nt, per k-step (K = 16) one
// 1-KiB piece; 16-KiB chunks of 16 pieces.  Pieces per layer: dense0 8 x 4, hidden 8 x 16, dense5 8 x 20, viewdirs 4 x 18
// (+ 8 zero pieces so that the stream ends on a chunk boundary).  64 points per wave, 256 per workgroup.
constexpr int kChunkBytesBf16V2 = 16384;
#ifndef NERF_BV2_RING_SLOTS
#define NERF_BV2_RING_SLOTS 3
#endif
constexpr int kRingSlotsBf16V2 = NERF_BV2_RING_SLOTS; // 3..8: chunk c + kRingSlots - 1 is DMA'd while chunk c is consumed (a chunk lasts ~0.45 us)
constexpr int kChunksSigmaBf16V2 = (32 + 4 * 128 + 160 + 2 * 128) / 16; // 60
constexpr int kChunksFullBf16V2 = kChunksSigmaBf16V2 + (128 + 72 + 8) / 16; // 73
constexpr int kLdsBytesBf16V2 = kRingSlotsBf16V2 * kChunkBytesBf16V2 + kSmallBytes;
constexpr int kPointsPerBlockBf16V2 = 256;

// ---- bf16x3 stream (mlp_kernel_bf16x3.hip, f32 by three-way bf16 split): the 16-bit pieces in the order
// (layer, k-step, output tile), each followed by the pieces of the second and third bf16 part of the same
// weights: a unit = 3 KiB, a k-step of an 8-tile layer = 24 KiB = one chunk, a k-step of viewdirs half a chunk.  No padding.
constexpr int kChunkBytesX3 = 24576;
#ifndef NERF_X3_RING_SLOTS
#define NERF_X3_RING_SLOTS 3
#endif
constexpr int kRingSlotsX3 = NERF_X3_RING_SLOTS; // 3..5 (measured equal: the kernel is power-limited, not latency-limited)
constexpr int kChunksSigmaX3 = 2 * 2 + 4 * 16 + 20 + 2 * 16;  // dense0 (2 tiles x 2 k-steps), dense1-4, dense5, dense6-7 = 120
constexpr int kChunksFullX3 = kChunksSigmaX3 + 16 + 9;        // + bottleneck + viewdirs (9 tiles, one chunk each) = 145
constexpr int kLdsBytesX3 = kRingSlotsX3 * kChunkBytesX3 + kSmallBytes;

// ---- f16x2 stream (mlp_kernel_f16x2.hip, f32 by two-way f16 split): the x3 stream's units with two pieces (the f16 parts w1, w2 of
// the same 32 x 16 weight block) instead of three: a unit = 2 KiB, a k-step of an 8-tile layer = 16 KiB = one chunk, a k-step of
// viewdirs half a chunk; the same chunk counts as the x3 stream.
constexpr int kChunkBytesF16X2 = 16384;
#ifndef NERF_F16X2_RING_SLOTS
#define NERF_F16X2_RING_SLOTS 4
#endif
constexpr int kRingSlotsF16X2 = NERF_F16X2_RING_SLOTS; // 3..6; a chunk lasts only 8 units x 3 MFMAs x 32 cycles = 0.35 us
constexpr int kChunksSigmaF16X2 = kChunksSigmaX3;
constexpr int kChunksFullF16X2 = kChunksFullX3;
constexpr int kLdsBytesF16X2 = kRingSlotsF16X2 * kChunkBytesF16X2 + kSmallBytes;

// feature held by register r (0..15) of a tile on lane-half h, relative to the tile's first feature
constexpr int regFeature(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// Encoding slots.  Points: 2 tiles; lane-half h computes octaves 5h..5h+4 (idx 0..29 = 6*o + {sin xyz, cos xyz}),
// idx 30/31 = raw x,y (h=0) or raw z, zero pad (h=1).  Returns the reference feature row
// (src/network.rs:263-292: [x,y,z] then per octave sin xyz, cos xyz) or -1 for the pad.
constexpr int posSlotFeature(int idx, int h) {
    return idx < 30 ? 3 + 6 * (5 * h + idx / 6) + idx % 6 : (h == 0 ? idx - 30 : (idx == 30 ? 2 : -1));
}
// Directions: 1 tile; half h computes octaves 2h..2h+1 (idx 0..11); h=0 idx 12..14 = raw x,y,z; rest pad.
constexpr int dirSlotFeature(int idx, int h) {
    return idx < 12 ? 3 + 6 * (2 * h + idx / 6) + idx % 6 : ((h == 0 && idx < 15) ? idx - 12 : -1);
}

} // namespace nerfmlp

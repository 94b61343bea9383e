// mlp_kernel.h -- launch interface of the fused MLP kernel (internal to libnerf_mi355x.so).
#pragma once
#include <hip/hip_runtime.h>

#include "mlp_layout.h"

enum { MLP_MODE_POINTS = 0, MLP_MODE_RAYS = 1, MLP_MODE_LIST = 2, MLP_MODE_GRID = 3 }; // LIST (f32 and split kernels): ray mode over a device-side list of sample indices (bit 31 of an entry: audited certificate)
// GRID (f32 sigma-only kernel, nerf_density_grid): the kernel makes its own points, slot i = cell (i % nx, (i / nx) % ny, i / (nx ny)) of a lattice

struct MlpArgs {
    const float *wstream;      // weight stream of the launched arithmetic (mlp_layout.h), device; f32 kernels: the FOLDED image (kChunksFullFolded)
    const float *small_params; // biases + head weights, kSmallFloats floats, device; f32 kernels: the folded image's (viewdirs bias = b')
    int n_points;
    int mode;
    // MLP_MODE_POINTS: forward_batch layouts (src/network.rs:197): points 3 x n SoA, dirs n x 3 AoS
    const float *pts_soa;
    const float *dirs_aos;
    // MLP_MODE_RAYS: point i = sample (i % samples_per_ray) of ray (i / samples_per_ray)
    const float *ray_dirs; // n_rays x 3, unit
    const float *t;        // n_rays x samples_per_ray
    int samples_per_ray;
    float origin[3];
    // outputs
    float *sigma_out; // n
    float *rgb_out;   // n x 3 (full kernels only)
    int skip_empty;                   // full kernels: skip the colour head of tiles whose 128 sigmas are all 0 (exact)
    unsigned long long *skip_counter; // optional: number of skipped 128-point tiles (atomic)
    unsigned long long *clock_out; // optional diagnostic: per workgroup {shader cycles, 100 MHz ticks} of the tile loop
    unsigned int *nonfinite;       // optional (split arithmetics): += points whose density pre-activation is NaN / inf (f16 range overflow)
    // zero certification (nerf_render_opts.certify_zero; nerf_render.cpp cert_pass): the bf16 kernel stores the density PRE-activation (no ReLU) in sigma_out ...
    int raw_pre;
    // ... and the f32 kernel evaluates only the listed samples (MLP_MODE_LIST: slot i -> sample point_list[i] = ray * samples_per_ray + k;
    // outputs are scattered to the sample's own position; n_points = capacity of the list, *point_list_count = its length)
    const unsigned int *point_list;
    const unsigned int *point_list_count;
    // optional second part of the list, filled from the END of the same buffer downwards (entry k at n_points - 1 - k): certify_zero puts the
    // listed samples that are probably zeros there (and the audited certificates), so that their tiles are all-zero and skip_empty skips
    // their colour heads.  Slots [0, front) map to entries [0, front), slots [front, front + back) to the last `back` entries.
    const unsigned int *point_list_count_back;
    // MLP_MODE_GRID (appended: the fields above keep their kernarg offsets): p = grid_lo + grid_step * (float)cell index, the multiply and
    // the add rounded separately (a host can restate the points bit for bit); n_points = nx * ny * nz.  sigma_out may be NULL.
    float grid_lo[3], grid_step[3];
    int grid_n[3];
    // fused occupancy (optional): word w = bit b set iff sigma of cell 32 w + b > occ_threshold (NaN: not occupied); ceil(n_points / 32) words,
    // every one of them written by the launch, the bits behind the last cell 0
    float occ_threshold;
    unsigned int *occ_bits;
    // f32 kernels (appended likewise): skip the MFMAs of k-steps whose ReLU'd B register is zero on all 64 lanes (mlp_f32_core.hip.h
    // tile_steps; bit-identical for a network whose parameters are all finite -- DevNet.zero_skip).  0: every k-step is executed.
    int zero_skip;
    unsigned long long *zskip_stats; // optional diagnostic (NERF_DEBUG_ZSKIP): {executed, total} ReLU k-steps of the launch, printed to stderr
    // f32 kernels, MLP_MODE_RAYS (appended likewise): ray grouping and wave tiling (mlp_layout.h ray_launch_slot).  The caller sets the two
    // switches (the context's, NERF_RAY_GROUPING / NERF_WAVE_TILING) and, for an image pass, rays_per_row; nerf_mlp_launch derives ray_map from
    // them and the launch's shape, whatever the caller left in it.
    int ray_grouping;   // 0: a workgroup tile is four consecutive wave tiles
    int wave_tiling;    // 0: a wave tile is 32 consecutive samples of one ray
    int rays_per_row;   // the launch's rays are whole rows of this many pixels; 0: unknown (caller-supplied ray batches), never tiled
    nerfmlp::RayLaunchMap ray_map;
    // MLP_MODE_LIST (appended likewise): per-ray origins of a certified ray batch, n_rays x 3, device; the point of list entry idx is
    // fl(ray_origins[idx / samples_per_ray] + fl(d * t)) per coordinate.  NULL: `origin` above.  No other mode reads it.
    const float *ray_origins;
    // f32 fused kernel, the full MLP_MODE_RAYS launch of an image pass (appended likewise): depth ordering (mlp_layout.h DepthOrder).  The caller
    // sets the context's switch (depth_order, NERF_DEPTH_ORDER) and, where nerf_mlp_depth_order says the launch qualifies, the pass's table
    // (sampling_kernels.h launch_depth_order: one slot per point of the ordered region); nerf_mlp_launch derives order_tiles / order_points and
    // the map of the rows behind the region.  order_table == NULL: today's static mapping.
    int depth_order;
    const unsigned int *order_table;
    int order_tiles, order_points;
    // f32 fused kernel, every mode: round k's tile of workgroup c is k G + ((c + k) mod G) (mlp_layout.h rotated_tile); 0: k G + c
    int tile_rotation;
    // full f32 and split-arithmetic kernels (appended likewise): take skip_empty's vote and skip path (a tile whose 128 sigmas are all 0 writes
    // rgb = 0 and skips the colour head; exact) without anything else that skip_empty means -- the launch keeps its mapping, depth ordering
    // included, and skip_counter stays NULL unless a diagnostic attaches it.  The host sets it for the full ray-mode launches of a plain render
    // (nerf_render.cpp eval_net; NERF_EMPTY_TILE_VOTE).
    int empty_vote;
    // f32 fused kernel, the sigma-only MLP_MODE_RAYS launch of a plain render whose densities only the resampler reads (appended likewise): the
    // coarse cut (mlp_layout.h RayCutWalk).  A workgroup walks the samples of an 8 x 4 pixel block front to back, four sample indices per tile,
    // keeps every ray's transmittance as the resampler will compute it (sample_alpha.hip.h) and leaves the block once all 32 rays are behind
    // the reference's T < 1e-4 cut; the samples it does not evaluate get sigma = 0 (the resampler gives them the weight 0 whatever they hold).
    // The host sets it in nerf_render.cpp eval_net alone (NERF_COARSE_CUT), where nerf_mlp_ray_cut says the launch qualifies, with the rays' far
    // and the context's counters: cut_counters[0] hands out the units (the launcher zeroes it in front of the launch), the u64 at
    // cut_counters + 2 counts the tiles not evaluated when cut_count is set (NERF_DEBUG_COARSE_CUT; the caller zeroes and reads it).
    int ray_cut;
    float ray_cut_far;
    unsigned int *cut_counters;
    int cut_count;
    // f32 fused kernel, the depth-ordered full MLP_MODE_RAYS launch of a plain image render whose sigma and rgb go to the pass's compositor
    // alone (appended likewise): the fine cut (mlp_layout.h fine_cut_walk_of).  A workgroup walks the ordered tiles of an 8 x 4 pixel block front
    // to back, keeps every ray's transmittance as k_composite will compute it (sample_alpha.hip.h) and leaves the block once all 32 rays are
    // behind the reference's T < 1e-4 cut; the table entries it does not evaluate get sigma = 0 and rgb = 0 (the compositor gives them the
    // weight 0 whatever they hold).  The host sets it in nerf_render.cpp eval_net alone (NERF_FINE_CUT) together with order_table, the table's
    // per-block words order_flags (k_depth_order: 1 = every row's keys ascend, so a ray's samples stand in index order; a block whose word is 0
    // is never left early), ray_cut_far and cut_counters, which the two cuts share: their launches are ordered on the stream.
    int fine_cut;
    const unsigned int *order_flags;
};

// The walk of a launch with these arguments under the coarse cut (n_points, samples_per_ray, rays_per_row, mode and the two switches
// wave_tiling / ray_grouping); blocks == 0: the launch does not qualify and keeps its static mapping.
inline nerfmlp::RayCutWalk nerf_mlp_ray_cut(const MlpArgs &a, bool full) {
    if (full || a.mode != MLP_MODE_RAYS || !a.cut_counters) return nerfmlp::RayCutWalk{0, 0, 0, 0};
    const nerfmlp::RayLaunchMap m = nerfmlp::ray_launch_map_of(a.n_points, a.samples_per_ray, a.rays_per_row, false, a.ray_grouping != 0, a.wave_tiling != 0);
    return nerfmlp::ray_cut_walk_of(nerfmlp::ray_cut_map_of(m), a.n_points);
}

// The walk of a launch with these arguments under the fine cut (the ordered region's blocks, then the tiles behind it one by one); blocks == 0:
// the launch does not qualify (no order table, no flags or no counters included) and keeps its rotated static walk.
inline nerfmlp::RayCutWalk nerf_mlp_fine_cut(const MlpArgs &a, bool full);

// The ordered region of a launch with these arguments (n_points, samples_per_ray, rays_per_row, mode, skip_empty and the two switches
// wave_tiling / depth_order); tiles == 0: the launch does not qualify and needs no table.
inline nerfmlp::DepthOrder nerf_mlp_depth_order(const MlpArgs &a, bool full) {
    return nerfmlp::depth_order_of(a.n_points, a.samples_per_ray, a.rays_per_row, full,
                                   a.mode == MLP_MODE_RAYS && a.depth_order != 0 && a.wave_tiling != 0 && a.skip_empty == 0);
}

inline nerfmlp::RayCutWalk nerf_mlp_fine_cut(const MlpArgs &a, bool full) {
    if (!full || !a.order_table || !a.order_flags || !a.cut_counters) return nerfmlp::RayCutWalk{0, 0, 0, 0};
    return nerfmlp::fine_cut_walk_of(nerf_mlp_depth_order(a, full).tiles, a.samples_per_ray, a.n_points);
}

// Sets the dynamic-LDS attribute of every kernel instantiation on the current device.
hipError_t nerf_mlp_init();
// full=false evaluates dense0..7 + alpha only (sigma); n_blocks = persistent workgroups (<= #CUs).  Sigma-only MLP_MODE_POINTS
// (nerf_density_batch) never reads dirs_aos; MLP_MODE_GRID exists sigma-only.
hipError_t nerf_mlp_launch(const MlpArgs &a, bool full, int n_blocks, hipStream_t stream);
// the zero-step diagnostic around a launch of an f32 kernel (no-ops when stats == NULL): clear the counters / read, synchronise and print them
hipError_t nerf_zskip_clear(unsigned long long *stats, hipStream_t stream);
hipError_t nerf_zskip_print(const char *what, unsigned long long *stats, hipStream_t stream);
// bf16-operand variant (mlp_kernel_bf16v2.hip): a.wstream is the output-tile-major stream (mlp_layout.h kChunks*Bf16V2)
hipError_t nerf_mlp_bf16v2_init();
hipError_t nerf_mlp_bf16v2_launch(const MlpArgs &a, bool full, int n_blocks, hipStream_t stream);
// mlp_kernel_f16v2.hip: the f16 twin of the bf16 kernel, sigma-only forms (certify_zero's pre-filter; MlpArgs / SeqArgs .nonfinite += tiles that left the f16 range)
hipError_t nerf_prefilter_f16v2_init();
hipError_t nerf_mlp_f16v2_launch(const MlpArgs &a, int n_blocks, hipStream_t stream);
// skip_dead in the bf16 arithmetic (same file): two ray cursors per wave; the trunk exports the bf16-packed relu(h8) of the live samples
// (512 B per sample; capacity nerf_seq_h8_bytes_bf16) for nerf_colour_bf16_launch.  SeqArgs / ColourArgs are declared below.
struct SeqArgs;
struct ColourArgs;
hipError_t nerf_seq_bf16_init();
size_t nerf_seq_h8_bytes_bf16(size_t n_samples);
hipError_t nerf_trunk_seq_bf16_launch(const SeqArgs &a, bool export_live, int n_blocks, hipStream_t stream);
hipError_t nerf_trunk_seq_f16v2_launch(const SeqArgs &a, int n_blocks, hipStream_t stream); // SeqArgs.prefilter only
hipError_t nerf_colour_bf16_launch(const ColourArgs &a, int n_blocks, hipStream_t stream);
// f32 by three-way bf16 split (mlp_kernel_bf16x3.hip): a.wstream is the three-part stream (mlp_layout.h kChunks*X3)
hipError_t nerf_mlp_bf16x3_init();
hipError_t nerf_mlp_bf16x3_launch(const MlpArgs &a, bool full, int n_blocks, hipStream_t stream);

// ---- exact dead-sample skipping (mlp_kernel_seq.hip for f32; mlp_split_kernels.hip.h for the split arithmetics) ------------
// Ray-sequential trunk: waves take rays from a device-side queue and walk each ray's samples front to back in chunks of 32,
// stopping at the reference's T < 1e-4 cut (src/lib.rs:276-279).  sigma_out must be zero-filled by the caller (samples behind
// the cut are never written).  With export_live the colour head runs on every sample with weight > 0:
//   f32 kernel            in the same launch (live samples compacted in LDS, colour passes of 32 columns): set rgb_out (zero-filled);
//   split arithmetics     trunk output to `h8` (compacted in HBM, 1 KiB per sample; capacity = all samples of the launch,
//                         nerf_seq_h8_bytes) for the second launch nerf_colour_*_launch;
//   bf16                  the same two-launch form with bf16-packed tiles (512 B per sample).
struct SeqArgs {
    const float *wstream;      // the f32 packed weight stream (sigma part is used)
    const float *small_params;
    int n_rays, samples_per_ray;
    const float *ray_dirs;     // n_rays x 3, unit
    const float *t;            // n_rays x samples_per_ray, ascending
    float origin[3];
    float far_;
    float *sigma_out;          // n_rays x samples_per_ray
    unsigned int *ray_counter; // zeroed before the launch
    unsigned int *live_count;  // zeroed before the launch (export_live): number of samples with weight > 0
    float *rgb_out;            // f32 kernel with export_live: n_rays x samples_per_ray x 3, zero-filled by the caller
    float *h8;
    unsigned int *slot_point;  // sample index (ray * samples_per_ray + k) of every exported slot
    unsigned long long *stats; // optional: += number of samples evaluated
    // hybrid sampling: evaluate only the rays of a device-side list (n_rays then only bounds the grid); retired rays zero-fill the
    // rest of their sigma row themselves (the row holds another arithmetic's values, the caller does not clear it)
    const unsigned int *ray_list;
    const unsigned int *ray_list_count;
    int zero_fill_after_cut;
    unsigned int *nonfinite;   // optional (split arithmetics): += points whose density pre-activation is NaN / inf
    // certify_zero's pre-filter (bf16 trunk only, export_live = false): store the density PRE-activation instead of sigma and retire a ray
    // once its bf16 transmittance falls below prefilter_cut_T (a prediction: kept below the reference's 1e-4 so that k_cert_plan's own
    // predicted cut always falls inside the evaluated samples).  The caller fills sigma_out with NaN (0xFF bytes): "not evaluated".
    int prefilter;
    float prefilter_cut_T;
    int zero_skip;                   // f32 trunk: as MlpArgs.zero_skip (appended: the fields above keep their kernarg offsets)
    unsigned long long *zskip_stats; // as MlpArgs.zskip_stats
    // 16-bit trunks without export (certify_zero's pre-filter; appended likewise): per-ray origins, n_rays x 3, device, read once per ray
    // when a wave takes it from the queue.  NULL: `origin` above.  The f32 and split trunks and the exporting forms never read it.
    const float *ray_origins;
};
struct ColourArgs {
    const float *wstream;      // the same stream (bottleneck + viewdirs part is used)
    const float *small_params;
    const unsigned int *live_count;
    const float *h8;
    const unsigned int *slot_point;
    const float *ray_dirs;
    int samples_per_ray;
    float *rgb_out;            // n x 3, scattered by sample index; zero-filled by the caller
    unsigned int *nonfinite;   // optional: += samples for which an operand left the arithmetic's range
};
hipError_t nerf_seq_init();
size_t nerf_seq_h8_bytes(size_t n_samples);
hipError_t nerf_trunk_seq_launch(const SeqArgs &a, bool export_live, int n_blocks, hipStream_t stream);
// the same two kernels in the bf16x3 arithmetic (mlp_kernel_bf16x3.hip): a.wstream is the three-part stream; the h8 tiles and
// the small parameters have the f32 kernels' layout
hipError_t nerf_seq_x3_init();
hipError_t nerf_trunk_seq_x3_launch(const SeqArgs &a, bool export_live, int n_blocks, hipStream_t stream);
hipError_t nerf_colour_x3_launch(const ColourArgs &a, int n_blocks, hipStream_t stream);
// f32 by two-way f16 split (mlp_kernel_f16x2.hip): a.wstream is the two-part f16 stream (mlp_layout.h kChunks*F16X2)
hipError_t nerf_mlp_f16x2_init();
hipError_t nerf_mlp_f16x2_launch(const MlpArgs &a, bool full, int n_blocks, hipStream_t stream);
hipError_t nerf_seq_f16x2_init();
hipError_t nerf_trunk_seq_f16x2_launch(const SeqArgs &a, bool export_live, int n_blocks, hipStream_t stream);
hipError_t nerf_colour_f16x2_launch(const ColourArgs &a, int n_blocks, hipStream_t stream);

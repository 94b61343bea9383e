/*
 * nerf_mi355x.h -- C ABI of libnerf_mi355x.so: the MI355X (gfx950) drop-in for the hot path of
 * elisabeth96/nerf-rs (ray-march + MLP forward + volume integration).
 *
 * The reference has no FFI on this path (it is a single Rust crate); the seams this ABI replaces are
 *   S2  Network::forward_batch(&self, points: &Matrix [3 x B, SoA], view_dirs: &[Vec3]) -> (Vec<Vec3>, Vec<f32>)
 *                                                                   reference src/network.rs:197-237
 *   S3  render_image(&Network, &Network, &Camera, fine_samples_per_ray) -> Vec<Vec3>
 *                                                                   reference src/lib.rs:474-565
 * plus the host-side pieces a caller needs around them (loader src/lib.rs:108-174, camera_from_samples
 * src/lib.rs:614-645, save_ppm src/lib.rs:567-580).  INTEGRATION.md shows the Rust `extern "C"` block a
 * maintainer of the reference would add to call these from src/lib.rs.
 *
 * Conventions: every function returns 0 on success or a negative nerf_status; nerf_last_error() gives the
 * message (the reference panics instead: src/lib.rs:36,118,127,483-501).  The caller owns all in/out buffers;
 * the context owns device memory.  Plain pointers and sizes only -- no C++ / torch types.  A context is bound to
 * one HIP device and is single-caller: one call at a time, and consecutive asynchronous calls (`*_device`) must use the
 * same stream or be separated by a stream synchronisation -- they share the context's pass workspace.  Create one
 * context per GPU / per thread.
 * All buffers at the boundary are f32 (the MLP arithmetic inside is selected by nerf_render_opts.mlp_dtype).  Without the HIP runtime or a gfx950 device nerf_create fails (there is no CPU fallback).
 */
#ifndef NERF_MI355X_H
#define NERF_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nerf_ctx nerf_ctx;

typedef enum {
    NERF_OK = 0,
    NERF_ERR_INVALID = -1,   /* bad argument (reference: assert!/panic) */
    NERF_ERR_IO = -2,        /* "read shapes"/"read tensor" (src/lib.rs:36,65) */
    NERF_ERR_MISSING = -3,   /* "missing matrix parameter"/"missing bias parameter" (src/lib.rs:118,127) */
    NERF_ERR_SHAPE = -4,     /* dims mismatch (debug_assert in src/lib.rs:119-120,128-129) */
    NERF_ERR_HIP = -5,       /* HIP runtime / device error */
    NERF_ERR_STATE = -6,     /* network not loaded */
    NERF_ERR_PARSE = -7      /* camera JSON malformed (src/lib.rs:620-631 unwrap/expect) */
} nerf_status;

enum { NERF_NET_COARSE = 0, NERF_NET_FINE = 1 };
enum { NERF_MLP_F32 = 0, NERF_MLP_BF16 = 1, NERF_MLP_BF16X3 = 2, NERF_MLP_F16X2 = 3 };

/* Mirrors `struct Camera` (src/lib.rs:197-211); samples_per_ray lives in nerf_render_opts.n_coarse.
 * alpha_* are the half field-of-view angles (radians); dir/up need not be orthogonal (basis is rebuilt
 * per src/lib.rs:216-218). */
typedef struct {
    int32_t nx, ny;
    float alpha_width, alpha_height;
    float pos[3], dir[3], up[3];
    float near_, far_;
} nerf_camera;

/* render_image's remaining inputs (src/lib.rs:474-482, 603-612) + the extensions BASELINE.json's configs need.
 * Zero-initialise, then set n_coarse (> 0).  The reference behaviour is n_coarse=64, n_fine=128, everything else 0. */
typedef struct {
    int32_t n_coarse;     /* camera.samples_per_ray */
    int32_t n_fine;       /* fine_samples_per_ray; 0 => fine net evaluated on the coarse samples only (src/lib.rs:295) */
    int32_t coarse_only;  /* ext: composite the coarse net's own rgb/sigma, skip the fine pass */
    int32_t crop_x0, crop_y0, crop_w, crop_h; /* ext: output window in pixels; crop_w = crop_h = 0 => full frame */
    int32_t ssaa;         /* ext: s x s rays per pixel, box filter; 0 or 1 => off */
    uint64_t seed;        /* counter-RNG seed (reference: unseeded thread_rng, src/lib.rs:375,407) */
    int32_t mlp_dtype;    /* ext: NERF_MLP_F32 (0, default: exact-f32 MFMA, the parity path) or NERF_MLP_BF16 (1: bf16
                           * operands / f32 accumulate on the bf16 matrix cores -- BASELINE config C5; PSNR-level parity).
                           * NERF_MLP_BF16X3 (2, opt-in): f32-accurate arithmetic on the bf16 matrix cores -- every weight and
                           * activation is split into three bf16 parts (exact to 2^-27) and a product is the sum of the six
                           * significant bf16 x bf16 products, accumulated in f32.  In a hierarchical render the coarse
                           * (sampling) pass stays on the exact-f32 kernel so that the fine sample positions equal the f32
                           * path's bit for bit; the fine (colour) pass runs in bf16x3.  Meets the f32 path's tolerances.
                           * NERF_MLP_F16X2 (3, opt-in): the cheaper sibling -- two f16 parts per operand (exact to 2^-22), three
                           * products per f32 product; same f32 sampling pass, same tolerances (the error against float64 stays
                           * at the f32 kernel's level: accumulation rounding dominates), half the matrix work of bf16x3.
                           * Range: f16 overflows at 65 504 -- activations must stay below it (true for the lego networks inside
                           * the scene and well beyond: validated for |p| <= 16; bf16x3 has no such limit); a network with a
                           * weight beyond the f16 range makes this mode unavailable (NERF_ERR_STATE). */
    int32_t skip_empty;   /* ext: 1 = skip the colour head (bottleneck + viewdirs + rgb: 17 % of a full MLP
                           * evaluation in the 16-bit arithmetics, 6.9 % in F32, whose kernels run the bottleneck folded into
                           * viewdirs) for every workgroup tile (128 samples in f32, 256 in bf16) whose densities are all 0.
                           * EXACT: such samples have alpha = 0 and weight 0, the image is bit-identical; only the work
                           * changes.  Default 0 so that timings are plain executed-FLOP figures. */
    int32_t skip_dead;    /* ext (the rest of it; every mlp_dtype): 1 = evaluate only what can reach a pixel.
                           * Rays are walked front to back in chunks of 32 samples; a ray is retired at the reference's
                           * T < 1e-4 cut (src/lib.rs:276-279: every later weight is exactly 0), and the colour head runs only
                           * on the samples whose weight is > 0 (F32: compacted in LDS, same launch; BF16 and the split arithmetics:
                           * compacted through an HBM buffer bounded by NERF_MAX_EXPORT_BYTES, second launch).  EXACT: the image is
                           * bit-identical to skip_dead = 0.  Takes precedence over skip_empty.  Default 0 so that timings are
                           * plain executed-FLOP figures; nerf_stats.n_exec_* report the evaluations actually executed. */
    int32_t hybrid_sampling; /* ext (needs skip_dead = 1, hierarchical render): 1 = run the SAMPLING (coarse) pass in a split
                           * arithmetic (the render's own; for an F32 render f16x2, or bf16x3 if the network exceeds the f16 range;
                           * the fine pass keeps mlp_dtype), then redo in exact f32 only the rays with an ill-conditioned
                           * hierarchical draw: one whose position is predicted to move by more than 1e-5 in t under the split
                           * arithmetic's density error (|dt| = bin width x |d cdf| / bin mass, |d cdf| bounded per bin edge to
                           * first order: light CDF bins, nearly empty rays),
                           * or whose transmittance passes within 0.1 % of the 1e-4 cut.  Those rays (18 % of the lego frame) get
                           * the f32 path's sample positions bit for bit; the others move by <= 1e-5 -- a bound under a measured
                           * model of the arithmetic's density error, not a proof: fuzzes of 700 M rays (tools/fuzz_hybrid_flags.py)
                           * found 0.9 unflagged rays per million beyond it, the largest at 2.8e-5.  Not bit-identical to
                           * hybrid_sampling = 0 (pixels differ by 2e-8 on average); held to the same Gate 1.
                           * nerf_stats.n_hybrid_rays = rays redone in f32. */
    int32_t certify_zero;  /* ext (ABI 4, reworked in ABI 5; mlp_dtype F32, BF16X3 or F16X2, no skip mode): 1 = a 16-bit pass over all samples (f16 operands where
                           * every weight and activation of the network fits the f16 range, else bf16; f32 accumulation either way) finds
                           * (Z) the samples whose density pre-activation is so far below 0 (per-network margin, see below) that the exact
                           * network's density is certainly 0 there as well, and predicts (C) where each ray's transmittance falls below the
                           * reference's 1e-4 cut (src/lib.rs:276-279: every later weight is zero-filled whatever its density).  The exact kernel
                           * -- for the fine pass of a split arithmetic that arithmetic's kernel -- evaluates only the other samples in front of
                           * the predicted cut (a device-side list: 7 % of the coarse, 15 % of the fine samples of the lego frame); the
                           * EXACT transmittance then confirms each cut, and where it does not (rare) the rest of that ray is evaluated in a
                           * second launch -- so (C) is exact by construction.  A certified sample has sigma = 0, weight 0 (src/lib.rs:271-272):
                           * the image is BIT-IDENTICAL to certify_zero = 0 as long as no certificate (Z) is wrong.
                           * (Z) rests on measurements, not on a proof, so it is AUDITED in every frame: a deterministic share of the certified samples (1 in 16 of those certified by
                           * less than twice the margin, 1 in 128 of the others) is evaluated
                           * exactly all the same; a positive density there (nerf_stats.n_certify_violations), or an audited sample on which the 16-bit
                           * pass was off by more than half the margin (nerf_stats.certify_max_error, certify_headroom), widens that network's margin for the life of
                           * the context (floors: 0.25 coarse, 0.5 fine with the f16 pass, 1.0 / 3.0 with the bf16 pass -- 2.5-9 x the largest difference to the
                           * exact pre-activation the audits see on certified samples of the lego networks; reset when a network is loaded) and the frame is rendered again (nerf_stats.n_certify_retries); if
                           * 8 widenings do not satisfy the audit the render fails with NERF_ERR_STATE.  An activation beyond 65 504 makes the f16 pass's
                           * pre-activations non-finite (never certified, counted): that network goes back to the bf16 pass for good and the frame is
                           * rendered again.  A network on which the 16-bit pass is less accurate
                           * thus calibrates itself, certifies nothing (random weights: pre-activations near 0), or fails loudly; what remains
                           * unobserved is a wrong certificate that is so rare that a 1-in-64 audit of ~1e8 certified samples per frame never
                           * meets one or its precursors.  Because of the audit a certify_zero render synchronises the stream before it returns
                           * (also nerf_render_image_device with stats == NULL).  nerf_stats.n_exec_* = samples the exact kernel evaluated. */
    /* ext (ABI 5): render only ONE BAND of the output window's rows (the whole window when band_count <= 1) -- what one GPU of several
     * renders (nerf_render_image_multi and nerf-rs_amd/distributed.py set these; reference counterpart: the rayon fan-out over blocks,
     * src/lib.rs:533-550, which balances by work stealing).  band_stripe_rows = 0: band band_index of band_count CONTIGUOUS bands (the
     * first rows % count bands one row longer) -- balanced when every ray costs the same.  band_stripe_rows = S > 0: the window's rows
     * are dealt out in stripes of S rows round-robin, this call renders the stripes band_index, band_index + band_count, ... -- balanced
     * also when rays differ in cost (skip_dead, certify_zero: the lego background, 75 % of the rays, is nearly free and sits in the top
     * rows).  rgb_out holds the band's rows PACKED, in frame order: nerf_band_rows(window rows, ...) x width x 3.  Every pixel is the same
     * bits as in a whole-window render (per-pixel counter RNG). */
    int32_t band_index, band_count, band_stripe_rows;
} nerf_render_opts;

/* Device-side timing of the last render (HIP events on the render stream). */
typedef struct {
    uint64_t n_rays, n_coarse_points, n_fine_points;
    double ms_total;       /* first kernel -> last kernel */
    double ms_coarse_mlp;  /* sum over passes */
    double ms_fine_mlp;
    double ms_other;       /* ray gen + sampling + compositing + downsample */
    uint32_t n_mlp_launches;
    uint32_t n_passes;
    uint64_t n_colour_skipped_points; /* samples whose colour head was skipped (skip_empty) */
    /* MLP evaluations actually executed (equal to the point counts above unless skip_empty / skip_dead removed work): */
    uint64_t n_exec_coarse_trunk;  /* coarse network, dense0..7 + alpha */
    uint64_t n_exec_fine_trunk;    /* fine network, dense0..7 + alpha */
    uint64_t n_exec_colour;        /* colour heads executed (fine network, or the coarse one when coarse_only): bottleneck + viewdirs + rgb; in F32
                                    * the bottleneck is folded into viewdirs at load time, a head is then viewdirs' + rgb */
    uint64_t n_hybrid_rays;        /* hybrid_sampling: rays whose coarse pass was redone in f32 (counted in n_exec_coarse_trunk too) */
    uint64_t n_nonfinite_points;   /* split arithmetics: evaluations in which an operand left the arithmetic's range (NERF_MLP_F16X2: an
                                    * activation beyond 65 504 -- every value is watched as it is split, one v_max3 per pair) or whose density
                                    * pre-activation was not finite.  0 in every validated configuration; non-zero means the frame is WRONG
                                    * there (f16 overflow yields finite garbage, not NaN): nerf_forward_batch_ex and every render that reads its
                                    * counters (nerf_render_image, nerf_render_image_multi, nerf_render_image_device with stats != NULL) fail
                                    * with NERF_ERR_STATE -- the stats are filled all the same. */
    /* certify_zero (ABI 5): the audit of the frame that was returned, see nerf_render_opts.certify_zero */
    uint64_t n_certify_audited;    /* certified samples that the exact kernel evaluated all the same (1 in 16 of those within twice the margin, 1 in 128 of the others) */
    uint64_t n_certify_violations; /* audited samples whose exact density was positive, summed over ALL renders of this frame (the last one had none) */
    uint32_t n_certify_retries;    /* times the frame was rendered again (margins widened after a failed audit, or the sample list enlarged) */
    uint32_t n_certify_fallback_rays; /* rays whose predicted cut the exact transmittance did not confirm (their remaining samples went through a second launch) */
    float certify_margin[2];       /* margins in force (coarse, fine network): a sample is certified iff its 16-bit (f16 / bf16 pass) pre-activation < -margin */
    float certify_headroom[2];     /* min over the audited samples of -(exact pre-activation): how far the closest one stood from a positive density (inf: none audited) */
    float certify_max_error[2];    /* max over the audited samples of |16-bit - exact pre-activation|: what the pre-filter got wrong on a sample it certified */
} nerf_stats;

/* ---- lifecycle ------------------------------------------------------------------------------------------ */
/* Environment read by nerf_create (per context; networks loaded into it afterwards follow it):
 *   NERF_ZERO_STEP_SKIP=0   the NERF_MLP_F32 kernels execute every MFMA k-step.  Default (unset or non-zero): a k-step of a 256-wide layer
 *                           whose ReLU'd inputs are zero for all 32 points of a wave is skipped -- exactly fma(a, 0, c) = c, so every output
 *                           keeps its bits; a network with a non-finite parameter runs with the skip off on its own.  Inputs and
 *                           activations need not be finite for that: subnormal, NaN, infinite and overflowing values give the same bits
 *                           with and without the skip (measured: profiles/zskip_counts.txt), whatever those bits are worth.
 *   NERF_RAY_GROUPING=0     ray-mode NERF_MLP_F32 launches give every 256-thread workgroup 128 consecutive samples.  Default: its four waves
 *                           take the same 32-sample segment of four neighbouring rays (whenever the samples per ray are a multiple of 32
 *                           and there are four rays), so that they skip alike and wait less for each other.  Which waves share a
 *                           workgroup changes no value: every output keeps its bits (nerf_debug_ray_grouping shows the mapping).
 *   NERF_WAVE_TILING=0      a wave of a ray-mode NERF_MLP_F32 launch holds 32 consecutive samples of one ray.  Default, for image renders (whole
 *                           rows of pixels; caller-supplied ray batches are never tiled) with samples per ray a multiple of 32: a wave holds a few
 *                           consecutive samples of each ray of a small block of neighbouring pixels (8 x 4 pixels x 1 sample in the density-only
 *                           sampling launch, 4 x 2 pixels x 4 samples in the launch that produces colours), whose points lie close together and
 *                           so have more dead hidden units in common for the zero-step skip.  Independent of NERF_RAY_GROUPING; every output
 *                           keeps its bits (nerf_debug_wave_tiling shows the mapping).
 *   NERF_DEPTH_ORDER=0      switches off depth ordering: in the f32 launch that produces the colours of an image pass (rows a multiple of 8 pixels
 *                           wide, at least 4 of them, samples per ray a multiple of 32 and at most 512; not skip_empty renders, not ray batches)
 *                           the samples of every 8 x 4 pixel block are merged by depth on the device and a wave holds 32 neighbours of that order,
 *                           not 4 samples of each ray of a 4 x 2 block: a ray places its importance samples where its own densities are, so only
 *                           depth says which samples of neighbouring rays lie together.  Off with NERF_WAVE_TILING=0 too; every output keeps
 *                           its bits (nerf_stage_depth_order shows the order).
 *   NERF_TILE_ROTATION=0    the persistent workgroups of the fused f32 kernel take tile k G + c in round k, not k G + ((c + k) mod G): the
 *                           rotation spreads tiles of systematically different cost (sample index, depth rank) over all workgroups.
 *   NERF_EMPTY_TILE_VOTE=0  the colour-producing ray-mode launches of a plain render (NERF_MLP_F32, NERF_MLP_BF16X3, NERF_MLP_F16X2; image renders
 *                           and ray batches with one origin) evaluate the colour head of every sample.  Default: the four waves of a workgroup
 *                           vote over the 128 densities of their tile, and a tile whose densities are all 0 writes rgb = 0 and skips the colour
 *                           head -- such samples have weight 0, every output keeps its bits.  skip_empty keeps its meaning (and its mapping);
 *                           n_colour_skipped_points of a plain render stays 0.
 *   NERF_COARSE_CUT=0       the density-only NERF_MLP_F32 sampling launch of a plain image render evaluates every coarse sample.  Default, where
 *                           only the resampler reads the launch's densities (not coarse_only, skip_dead, certify_zero or n_fine = 0 renders, not
 *                           ray batches) and the launch is tiled 8 x 4 pixels x 1 sample (see NERF_WAVE_TILING): a workgroup walks the samples of
 *                           a pixel block front to back, keeps each ray's transmittance as the resampler will compute it, and leaves the block
 *                           once all its 32 rays are behind the reference's T < 1e-4 cut -- the resampler gives every sample behind the cut the
 *                           weight 0 whatever its density, so every output keeps its bits.  The NERF_MLP_BF16X3 / NERF_MLP_F16X2 renders' f32
 *                           sampling launch takes it too.  The tiles of such a launch are not grouped (NERF_RAY_GROUPING).  A cut launch hands
 *                           out whole pixel blocks, so only launches of at least 16 blocks per compute unit are cut (131 072 rays on 256 units:
 *                           fewer would leave workgroups idle); NERF_COARSE_CUT=2 cuts every qualifying launch (tests, diagnostics).
 *   NERF_FINE_CUT=0         the depth-ordered full NERF_MLP_F32 launch of a plain image render evaluates every sample.  Default, where the
 *                           launch's densities and colours go to the pass's compositor and nowhere else (the fine pass, or the coarse network's
 *                           launch of a coarse_only render; not skip_empty, skip_dead or certify_zero renders, not ray batches, not the stage
 *                           calls) and the rays end at the camera's far: a workgroup walks the ordered tiles of an 8 x 4 pixel block front to
 *                           back, keeps each ray's transmittance as the compositor will compute it, and leaves the block once all its 32 rays
 *                           are behind the reference's T < 1e-4 cut -- the compositor gives every sample behind the cut the weight 0 whatever
 *                           its density and colour, so every output keeps its bits.  Whole blocks are handed out, and a fine block is three
 *                           times as long as a coarse one: only launches of at least 48 blocks per compute unit are cut (393 216 rays on 256
 *                           units); NERF_FINE_CUT=2 cuts every qualifying launch (tests, diagnostics).
 *   NERF_DEBUG_ZSKIP=1      diagnostic: every f32 MLP launch synchronises and prints its executed / total ReLU k-steps to stderr.  The counters
 *                           describe the dense colour head and every sample: such a context runs without the empty-tile vote and the two cuts.
 *   NERF_DEBUG_FINE_CUT=1   diagnostic: every launch that takes the fine cut synchronises and prints "nerf fine cut: nerf_mlp_kernel<full,rays>
 *                           tiles_skipped=N tiles=M blocks=B" to stderr.
 *   NERF_DEBUG_COARSE_CUT=1  diagnostic: every launch that takes the coarse cut synchronises and prints "nerf coarse cut: nerf_mlp_kernel<sigma,rays>
 *                           tiles_skipped=N tiles=M blocks=B" to stderr.
 *   NERF_DEBUG_EMPTY_TILES=1  diagnostic: every launch that takes the empty-tile vote synchronises and prints "nerf empty tiles: <kernel>
 *                           tiles_skipped=N tiles=M" to stderr.
 *   NERF_DEBUG_CLOCK=1      diagnostic: nerf_debug_shader_clock_mhz, nerf_debug_workgroup_clocks of the fine launch; 2: of the sampling launch. */
int nerf_create(int device_id, nerf_ctx **out);
void nerf_destroy(nerf_ctx *ctx);
/* Message of the last failing call on ctx (or of the last failing context-free call when ctx == NULL). */
const char *nerf_last_error(const nerf_ctx *ctx);
int nerf_device_info(const nerf_ctx *ctx, int *n_cus, char *arch_name, size_t arch_name_len);

/* ---- loader: load_network_from_dir (src/lib.rs:108-174), same directory format (shapes.txt + <name>.bin,
 * little-endian f32, kernels [in][out] row-major), same required tensor names, same failure cases ---------- */
int nerf_load_network_dir(nerf_ctx *ctx, int which, const char *dir);
/* For hosts that read the tensors themselves (Rust load_tensor): n named tensors, dims[2*i], dims[2*i+1]
 * (second = 0 for biases). */
int nerf_load_network_tensors(nerf_ctx *ctx, int which, int n, const char *const *names, const int64_t *dims,
                              const float *const *data);

/* Packed weight blob: the pre-padded, pre-permuted device image of one network in a single file, so
 * that start-up is one read + one memcpy.  nerf_pack_network_dir converts the reference's directory format (host-only);
 * nerf_load_network_blob uploads it.  The directory loader stays the compatibility path.  Blob layout: 16-byte header
 * {"NRFMI355", u32 version = 1, u32 n_floats} + the weight stream + the small-parameter block (mlp_layout.h). */
int nerf_pack_network_dir(const char *dir, const char *blob_path);
int nerf_load_network_blob(nerf_ctx *ctx, int which, const char *blob_path);

/* Host-only validation of a weight directory (same checks as nerf_load_network_dir, no device needed). */
int nerf_check_network_dir(const char *dir);
/* Host-only validation of a packed blob (same reader and checks as nerf_load_network_blob: magic, version, exact size). */
int nerf_check_network_blob(const char *blob_path);
/* Diagnostic: the packed device images of a weight directory (layout: nerf-rs_amd/csrc/mlp_layout.h).  Pass NULL
 * buffers to query the lengths (in floats).  Host-only. */
int nerf_debug_pack_network_dir(const char *dir, float *wstream, size_t wstream_cap, float *small, size_t small_cap,
                                size_t *wstream_len, size_t *small_len);
/* Diagnostic: the image the NERF_MLP_F32 kernels read, formed from the packed one at load time (directory and blob loaders alike):
 * the bottleneck layer has no activation and feeds only the viewdirs layer, so the two are one linear map W' = W_b . W_v[0:256],
 * b' = b_v + b_b^T . W_v[0:256] (fp64 accumulation, rounded once to f32).  129 chunks instead of 145 (mlp_layout.h
 * kChunksFullFolded); the small block differs in the viewdirs bias only.  Same calling convention as above.  Host-only. */
int nerf_debug_fold_network_dir(const char *dir, float *wstream, size_t wstream_cap, float *small, size_t small_cap,
                                size_t *wstream_len, size_t *small_len);
/* Diagnostic: one of the four 16-bit weight streams every loader builds from the packed image (layouts: nerf-rs_amd/csrc/mlp_layout.h), as raw
 * 16-bit patterns: NERF_STREAM_BF16V2 (NERF_MLP_BF16), NERF_STREAM_F16V2 (certify_zero's f16 pre-filter), NERF_STREAM_BF16X3, NERF_STREAM_F16X2.
 * *n = its length in elements, *available = 0 and *n = 0 if a weight exceeds the f16 range (the two f16 streams only; nothing is written).
 * out == NULL queries; a buffer of cap < *n elements is refused with NERF_ERR_INVALID and left untouched.  n, available may be NULL.  Host-only. */
enum { NERF_STREAM_BF16V2 = 0, NERF_STREAM_F16V2 = 1, NERF_STREAM_BF16X3 = 2, NERF_STREAM_F16X2 = 3 };
int nerf_debug_network_stream_dir(const char *dir, int kind, uint16_t *out, size_t cap, size_t *n, int *available);
/* Diagnostic: what the loaders decide for zero-step skipping of the NERF_MLP_F32 kernels (see NERF_ZERO_STEP_SKIP at nerf_create): *eligible = 1 iff
 * every value of the folded image of this weight directory is finite.  Host-only: it reports the loaders' predicate, not a context; what a
 * context did with a loaded network shows in NERF_DEBUG_ZSKIP's counters (executed == total: every k-step was executed). */
int nerf_debug_zero_skip_network_dir(const char *dir, int *eligible);
/* Diagnostic: the three bf16 parts (raw bit patterns) the NERF_MLP_BF16X3 packer stores for each of n f32 weights:
 * parts[3 i + k], k = 0..2, with v = p0 + p1 + p2 up to 2^-27 |v|.  Host-only. */
int nerf_debug_split_bf16x3(const float *values, size_t n, uint16_t *parts /* 3 n */);
/* Diagnostic: certify_zero's audit policy as the renderer applies it after every certified frame, per network -- given the margin in force and
 * what the audit found (audited certificates, violations among them, least headroom, largest |bf16 - exact| error: the nerf_stats fields),
 * returns 0 if the frame stands, else 1 (a violation: margin x 4, or 4 x the error), 2 (headroom below half the margin: x 2, or 4 x the
 * error) or 3 (error above half the margin: x 1.25, or 3 x the error) with the widened margin in *new_margin.  Host-only. */
int nerf_debug_certify_policy(float margin, uint64_t audited, uint64_t violations, float headroom, float max_error, float *new_margin);
/* The same for the NERF_MLP_F16X2 packer: two f16 parts (IEEE binary16 bit patterns), v = p0 + p1 up to 2^-22 |v|.  Host-only. */
int nerf_debug_split_f16x2(const float *values, size_t n, uint16_t *parts /* 2 n */);
/* Diagnostic: which samples the waves of a ray-mode NERF_MLP_F32 launch of n_rays x samples_per_ray samples evaluate (see NERF_RAY_GROUPING at
 * nerf_create; `enabled`: the context's switch).  For every workgroup tile T = 0 .. ceil(n_rays samples_per_ray / 128) - 1 and wave w = 0..3,
 * first_slot_of_wave_tile[4 T + w] = first of the wave's 32 consecutive sample slots (slot = ray * samples_per_ray + sample), from the function
 * the kernel calls.  Grouped (enabled, samples_per_ray a multiple of 32, n_rays >= 4): wave w of tile T = b S + j, S = samples_per_ray / 32,
 * j < S, b < n_rays / 4, holds segment j of ray 4 b + w; the last n_rays % 4 rays and every other launch: slot 128 T + 32 w.  Host-only. */
int nerf_debug_ray_grouping(int n_rays, int samples_per_ray, int enabled, int32_t *first_slot_of_wave_tile);
/* Diagnostic: the same for an image pass of `rows` whole rows of rays_per_row rays, lane by lane (see NERF_WAVE_TILING at nerf_create;
 * ray_grouping, wave_tiling: the context's two switches; full: 1 for a launch that also produces colours, 0 for the density-only sampling
 * launch -- the two kinds start from different pixel blocks).  For every workgroup tile T, wave w = 0..3 and lane p = 0..31,
 * slot[(4 T + w) 32 + p] = the sample slot (ray * samples_per_ray + sample, rays row-major) that lane evaluates, or -1 for a padding lane
 * of the launch's last tile; from the functions the kernel calls.  With wave_tiling = 0, or where a launch is not tiled (samples_per_ray no
 * multiple of 32, fewer rows than the block is high, no block of 4 pixels whose width divides rays_per_row), it is nerf_debug_ray_grouping's
 * table spelled out: first slot + p.  Host-only. */
int nerf_debug_wave_tiling(int rows, int rays_per_row, int samples_per_ray, int full, int ray_grouping, int wave_tiling, int32_t *slot);
/* Which persistent workgroup of n_workgroups takes which of n_tiles workgroup tiles of a fused f32 launch, and in which of its rounds: the
 * kernel's own tile walk run on the host (rotation != 0: round k's tile of workgroup c is k G + ((c + k) mod G); 0: k G + c).  Both
 * tables hold n_tiles entries; a tile nobody takes keeps -1, a tile taken twice -2 (neither may occur).  No device needed. */
int nerf_debug_tile_rotation(int n_tiles, int n_workgroups, int rotation, int32_t *workgroup_of_tile, int32_t *round_of_tile);
/* The order in which the density-only sampling launch of an image pass of `rows` whole rows of rays_per_row rays walks its workgroup tiles
 * under the coarse cut (see NERF_COARSE_CUT at nerf_create; ray_grouping: the context's switch, which the rows behind the pixel blocks keep):
 * the kernel's own unit-to-tile functions run on the host, unit after unit.  *blocks = the launch's 8 x 4 pixel blocks, each *block_tiles =
 * samples_per_ray / 4 consecutive tiles of nerf_debug_wave_tiling's table with ray_grouping = 0 (wave w of a block's tile k: sample index
 * 4 k + w of its 32 rays); the tiles behind them are units of their own.  Block cut_block is taken to be cut behind its tile cut_after
 * (0-based; cut_block < 0: no block is cut) and the walk leaves it there.  tiles[i] = the i-th tile visited; returns how many were (a negative
 * value: an error code), at most ceil(rows rays_per_row samples_per_ray / 128) <= tiles_cap.  *blocks = 0: the launch does not qualify for the
 * cut (samples_per_ray no multiple of 32, fewer than 4 rows, rays_per_row no multiple of 8) and the table is 0, 1, 2, ...  blocks, block_tiles
 * may be NULL.  No device needed. */
int nerf_debug_coarse_cut_walk(int rows, int rays_per_row, int samples_per_ray, int ray_grouping, int cut_block, int cut_after, int32_t *tiles,
                               size_t tiles_cap, int32_t *blocks, int32_t *block_tiles);

/* The same for the depth-ordered full launch of an image pass under the fine cut (see NERF_FINE_CUT at nerf_create): *blocks = the launch's
 * 8 x 4 pixel blocks over its first (rows / 4) * 4 rows, each *block_tiles = samples_per_ray / 4 consecutive tiles -- block b's part of the
 * order table (nerf_stage_depth_order), entries 128 T .. 128 T + 127 per tile T, front to back; the tiles of the rows behind them are units
 * of their own.  Block cut_block is taken to be cut behind its tile cut_after, as above.  *blocks = 0: the launch is not depth-ordered
 * (samples_per_ray no multiple of 32 or above 512, fewer than 4 rows, rays_per_row no multiple of 8) and the table is 0, 1, 2, ...  No device
 * needed. */
int nerf_debug_fine_cut_walk(int rows, int rays_per_row, int samples_per_ray, int cut_block, int cut_after, int32_t *tiles, size_t tiles_cap,
                             int32_t *blocks, int32_t *block_tiles);

/* ---- S2: Network::forward_batch (src/network.rs:197-237) -------------------------------------------------- */
/* host pointers, synchronous.  n == 0 is a no-op (src/network.rs:199-201).
 * Input domain: the positional encoding evaluates sin/cos(2^k p), k <= 9, with a branch-free three-constant Cody-Waite
 * reduction that is accurate (<= 1.2e-7 absolute) for |2^9 p| <= 2^20, i.e. |p| <= 2048 per coordinate -- three orders of
 * magnitude beyond the scene (|p| <= 2.42 in the lego frustum); beyond that the accuracy degrades gradually, nothing faults.
 * n is limited to INT32_MAX minus one grid stride of tiles (~2.1e9 points); larger batches return NERF_ERR_INVALID. */
int nerf_forward_batch(nerf_ctx *ctx, int which, const float *pts_soa /*3 x n*/, const float *dirs_aos /*n x 3*/,
                       size_t n, float *rgb_aos /*n x 3*/, float *sigma /*n*/);
/* same with an explicit MLP arithmetic (NERF_MLP_F32 / NERF_MLP_BF16 / NERF_MLP_BF16X3 / NERF_MLP_F16X2).  In the two split
 * arithmetics a density of 0 whose pre-activation lies within 4e-5 of 0 is returned as -0.0f (an "uncertain zero": the f32
 * kernel may see a tiny positive density there; numerically it IS 0 -- hybrid_sampling's flag reads the sign). */
int nerf_forward_batch_ex(nerf_ctx *ctx, int which, int mlp_dtype, const float *pts_soa, const float *dirs_aos, size_t n,
                          float *rgb_aos, float *sigma);
/* device pointers, asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream) */
int nerf_forward_batch_device(nerf_ctx *ctx, int which, const float *d_pts_soa, const float *d_dirs_aos, size_t n,
                              float *d_rgb_aos, float *d_sigma, void *stream);

/* ---- density queries: sigma alone, at caller points or on a lattice the kernel generates itself ------------------------------ */
/* sigma of network `which` at n points (3 x n SoA as nerf_forward_batch): the same bits nerf_forward_batch returns as sigma (density does
 * not depend on the view direction, src/network.rs:197-237: it is read off dense7 before the direction is concatenated), without a
 * direction per point and without the colour head.  f32 arithmetic only.  Host pointers, synchronous; n == 0 is a no-op.  Input domain
 * and largest n: as nerf_forward_batch (|p| <= 2048 per coordinate for full accuracy; beyond that the accuracy degrades, nothing faults). */
int nerf_density_batch(nerf_ctx *ctx, int which, const float *pts_soa /*3 x n*/, size_t n, float *sigma /*n*/);
/* device pointers, asynchronous on `stream` */
int nerf_density_batch_device(nerf_ctx *ctx, int which, const float *d_pts_soa, size_t n, float *d_sigma, void *stream);
/* sigma on the lattice p = lo + step * (ix, iy, iz), 0 <= i* < dims[*]: per coordinate the f32 product step * (float)i, then the f32 sum
 * with lo, each rounded once -- a host that builds the points the same way gets the bits of nerf_density_batch.  The points are made
 * inside the kernel: nothing but the weights is read.  step may be 0 or negative.  N = dims[0] dims[1] dims[2] is one launch: at most the
 * largest n of nerf_forward_batch.  The lattice should stay inside nerf_forward_batch's input domain.
 *   sigma_out  dims[2] x dims[1] x dims[0] floats, x fastest (linear cell ix + dims[0] (iy + dims[1] iz)), or NULL
 *   occ_bits   ceil(N / 32) uint32 words, bit b of word w = (sigma of linear cell 32 w + b) > threshold (a NaN sigma is not occupied;
 *              the bits behind cell N - 1 are 0), or NULL; threshold must be >= 0 (not NaN) when occ_bits is given.  An occupancy-only
 *              query never materialises sigma: N / 8 bytes instead of 4 N
 *   n_occupied number of set bits; bounds = {ix_min, iy_min, iz_min, ix_max, iy_max, iz_max} of the set cells, inclusive (no set cell:
 *              mins = dims, maxs = -1).  Both optional, only with occ_bits.
 * At least one of sigma_out, occ_bits.  f32 arithmetic only.  Host pointers, synchronous. */
int nerf_density_grid(nerf_ctx *ctx, int which, const float lo[3], const float step[3], const int32_t dims[3], float *sigma_out,
                      float threshold, uint32_t *occ_bits, uint64_t *n_occupied, int32_t bounds[6]);
/* d_sigma_out / d_occ_bits: device pointers; n_occupied / bounds: HOST pointers.  Asynchronous on `stream` unless n_occupied or bounds
 * is given: then the call synchronises the stream before it returns. */
int nerf_density_grid_device(nerf_ctx *ctx, int which, const float lo[3], const float step[3], const int32_t dims[3],
                             float *d_sigma_out, float threshold, uint32_t *d_occ_bits, uint64_t *n_occupied, int32_t bounds[6],
                             void *stream);

/* ---- isosurface meshes: the level set sigma = iso of a density lattice as a deterministic, welded, indexed triangle mesh ----------------
 * Marching tetrahedra on the Kuhn split of every lattice cell, on the device (nerf-rs_amd/csrc/isosurface_kernels.hip).  The split uses
 * the same face diagonal on both sides of every cell face: the surface is watertight by construction and no case is ambiguous.  Every
 * output position is fixed by prefix sums (no atomics): the same input gives the same bits in every run.  A host can restate the output
 * bit for bit from the following conventions (tests/helpers/marching_tets.py does).
 * LATTICE   the points of nerf_density_grid: p = lo + step * index, per coordinate the f32 product step * (float)i, then the f32 sum with lo,
 *           each rounded once; sigma is dims[2] x dims[1] x dims[0] floats, x fastest (linear index A = ix + dims[0] (iy + dims[1] iz)).
 *           Every dims[k] >= 2, every step[k] != 0; lo, step and iso finite; N = dims[0] dims[1] dims[2] at most the smaller of 2^28 and
 *           nerf_forward_batch's largest n (every count then fits 32 bits) -- anything else is NERF_ERR_INVALID, checked before the context or
 *           the device is needed.  step may be negative.
 * INSIDE    sigma > iso, the occupancy predicate; a NaN is not inside.
 * VERTICES  each lattice point A owns up to 7 edges, to A + d for d = (dx, dy, dz) in {0,1}^3 \ {0} where A + d lies on the lattice (3 axis
 *           edges, 3 face diagonals, the body diagonal: the edges of the Kuhn tetrahedra).  An edge carries one vertex iff both end sigma
 *           are finite and exactly one end is inside.  Vertex ids ascend with A, within A with dx + 2 dy + 4 dz.  With B = A + d:
 *             t = (iso - sigma_A) / (sigma_B - sigma_A)      two f32 subtractions, one correctly rounded f32 division
 *             p = p_A + t * (p_B - p_A) per coordinate       subtract, multiply, add, each rounded once
 *           always evaluated from A to B, so that every cell sharing the edge sees the same bits.
 * TRIANGLES cells ascend in linear index ix + (dims[0] - 1) (iy + (dims[1] - 1) iz); a cell with a non-finite corner emits nothing.
 *           Within a cell with low corner c the six tetrahedra (c, c + e_a, c + e_a + e_b, c + (1,1,1)) follow in the axis orders
 *           (a, b, .) = xyz, xzy, yxz, yzx, zxy, zyx.  A tetrahedron with one corner inside, or one corner outside, gives one triangle; two
 *           corners inside give a quad, stored as two triangles.  Winding: counter-clockwise seen from the outside (sigma <= iso) IN
 *           LATTICE INDEX SPACE -- independent of lo and step; a lattice with an odd number of negative steps is therefore wound INWARDS
 *           in world space (flip the triangles, or mirror the lattice, if that matters).  Canonical form: a triangle starts with its
 *           smallest vertex id; a quad's four vertices are taken in their cyclic order under that winding starting at the smallest id m
 *           and split along the diagonal through m: (m, q1, q2), then (m, q2, q3).  Indices are uint32, three per triangle.
 * NORMALS   per lattice point P and axis k: g_k = (sigma(P + e_k) - sigma(P - e_k)) / (x_k(P + e_k) - x_k(P - e_k)), indices clamped to the
 *           lattice (one-sided at the borders), x_k the lattice coordinates above; at a vertex g = g_A + t * (g_B - g_A) with the arithmetic
 *           of the position; len = sqrt((g_x^2 + g_y^2) + g_z^2), every operation rounded once, sqrt and division correctly rounded;
 *           n = (-g) / len, the unit normal towards lower density; n = (0, 0, 0) where len is 0 or not finite.
 * COLOURS   (network entry points) the rgb nerf_forward_batch of the same network returns at the vertex positions with dirs = -n (the
 *           surface seen head-on; where n is zero the zero vector, negated, is passed); f32, n_vertices x 3.
 * OUTPUT    vertices, normals, rgb: n_vertices x 3 floats; triangles: n_triangles x 3 uint32; each may be NULL.  n_vertices and
 *           n_triangles are required and always returned.  The arrays are written only when BOTH counts fit their capacities
 *           (cap_vertices vertices, cap_triangles triangles); otherwise nothing is written and the call still returns NERF_OK: all-NULL
 *           arrays with zero capacities is the size query (a query followed by a fill runs everything twice, the network's lattice
 *           evaluation included).
 * Workspace: 16 bytes per lattice point in the context (sigma, one classification word, two prefix sums: 268 MB for 256^3), grown on
 * demand -- a warm call allocates nothing; the sigma lattice of nerf_extract_mesh lives there and never reaches the host. */
/* the caller's sigma lattice (host); needs a context, not a network */
int nerf_isosurface_grid(nerf_ctx *ctx, const float *sigma, const float lo[3], const float step[3], const int32_t dims[3], float iso,
                         float *vertices, float *normals, size_t cap_vertices, uint32_t *triangles, size_t cap_triangles,
                         uint64_t *n_vertices, uint64_t *n_triangles);
/* sigma of network `which` evaluated in grid mode (nerf_density_grid's launch) into the workspace, then the same kernels (+ colours).
 * Host pointers, synchronous.  NERF_ERR_STATE: network not loaded. */
int nerf_extract_mesh(nerf_ctx *ctx, int which, const float lo[3], const float step[3], const int32_t dims[3], float iso,
                      float *vertices, float *normals, float *rgb, size_t cap_vertices, uint32_t *triangles, size_t cap_triangles,
                      uint64_t *n_vertices, uint64_t *n_triangles);
/* device output pointers, on `stream`; n_vertices / n_triangles are HOST pointers: the call synchronises the stream to read the counts,
 * the emitting kernels that follow are asynchronous */
int nerf_extract_mesh_device(nerf_ctx *ctx, int which, const float lo[3], const float step[3], const int32_t dims[3], float iso,
                             float *d_vertices, float *d_normals, float *d_rgb, size_t cap_vertices, uint32_t *d_triangles,
                             size_t cap_triangles, uint64_t *n_vertices, uint64_t *n_triangles, void *stream);

/* ---- lattice components: the connected pieces of the inside points of a density lattice, and meshes of the largest pieces only ---------------
 * A NeRF density has floaters: specks of sigma > iso detached from the object.  These entry points label the pieces on the device
 * (nerf-rs_amd/csrc/components_kernels.hip), rank them by size, and let the mesh entry points drop all but the kept ones, without the lattice
 * or the mesh visiting the host.  A host can restate every output bit for bit from the following (tests/helpers/lattice_components.py does).
 * LATTICE       as above (x fastest, linear index A = ix + dims[0] (iy + dims[1] iz)); nerf_lattice_components needs no lo / step and accepts
 *               every dims[k] >= 1; N as for the meshes (at most 2^28 and nerf_forward_batch's largest n); iso finite.
 * INSIDE        sigma > iso, the predicate of the meshes: a NaN is not inside, +inf is.
 * CONNECTIVITY  two inside points are adjacent iff they are the two ends of a Kuhn edge: they differ by +d or -d for one d in {0,1}^3 \ {0} --
 *               the 7 edges a point owns and the 7 it is the far end of, 14 neighbours.  (0,0,0)-(1,1,1) are adjacent, (1,0,0)-(0,1,0) are not.
 *               This is the connectivity of the piecewise-linear level set the mesh triangulates (sigma is linear along an edge of a
 *               tetrahedron, so two inside ends are joined inside); 6, 18 or 26 neighbours would disagree with the mesh.
 * LABEL         of a component: the smallest linear index among its points; of a point that is not inside: 0xFFFFFFFF.
 * SIZE, RANK    n_points = number of lattice points of the component; components are ordered by n_points descending, ties by label ascending.
 * FILTER        nerf_component_filter {keep_largest, min_points}: a component is KEPT iff n_points >= min_points and (keep_largest == 0 or its
 *               rank < keep_largest).  keep_largest > 64 is NERF_ERR_INVALID.  A NULL filter or {0, 0} keeps everything.
 * FILTERED MESH a point of a discarded component counts as NOT INSIDE when edges and cells are classified; nothing else changes: t, positions
 *               and normals come from the true sigma with the arithmetic above.  The four corners of a tetrahedron are pairwise Kuhn-adjacent,
 *               so its inside corners are all kept or all discarded.  The filtered mesh is therefore exactly the unfiltered mesh minus the
 *               triangles of discarded components, minus the vertices whose inside end belongs to a discarded component, the remaining vertex
 *               ids renumbered in their old order: vertex bits and triangle order are unchanged.  With a NULL or {0, 0} filter the output is
 *               that of the unfiltered entry point, bit for bit.  The capacity protocol is the existing one, applied to the filtered counts.
 * The labels are the same bits in every run (the root of a component is its smallest index whatever order the device's atomics land in);
 * sizes, counts and bounds are integer sums, minima and maxima.  No kernel waits for another workgroup.
 * Workspace: 8 bytes per lattice point (label; size + keep flag) on top of the meshes' 16, in the context, grown on demand, and only when a
 * filter, a count or a component query is asked for -- a warm call allocates nothing.
 * The struct arguments are declared `const void *` / `void *` below so that bindings generated from the scalar types alone keep working;
 * they point to the two structs defined here.  This gives up type checking for C and C++ callers: to be revisited (typed pointers, an
 * ABI-compatible change) once the textual check of the bindings against this header knows the two struct names. */
typedef struct { uint32_t keep_largest, min_points; } nerf_component_filter;           /* 8 bytes */
typedef struct { uint32_t label, n_points; int32_t bounds[6]; } nerf_component;        /* 32 bytes; bounds as nerf_density_grid: inclusive
                                                                                        * {ix_min, iy_min, iz_min, ix_max, iy_max, iz_max} */
/* Labels every point of the caller's lattice (host, dims[2] x dims[1] x dims[0] floats).  labels_out (N uint32) and table (nerf_component
 * [cap_table]; receives the first min(cap_table, n_components) components in rank order, nothing beyond) are optional; n_components is
 * required.  cap_table <= 64; a table with cap_table == 0 is NERF_ERR_INVALID.  Needs a context, not a network.  Synchronous. */
int nerf_lattice_components(nerf_ctx *ctx, const float *sigma, const int32_t dims[3], float iso, uint32_t *labels_out, void *table,
                            size_t cap_table, uint64_t *n_components);
/* d_sigma / d_labels_out: device pointers; table and n_components: HOST pointers -- the call synchronises the stream to return them.  After
 * nerf_density_grid_device on the same stream sigma never reaches the host. */
int nerf_lattice_components_device(nerf_ctx *ctx, const float *d_sigma, const int32_t dims[3], float iso, uint32_t *d_labels_out, void *table,
                                   size_t cap_table, uint64_t *n_components, void *stream);
/* nerf_isosurface_grid / nerf_extract_mesh / nerf_extract_mesh_device restricted to the kept components.  filter: const nerf_component_filter *
 * or NULL.  n_components (all components of the lattice) and n_kept (those that pass the filter) are optional HOST pointers. */
int nerf_isosurface_grid_filtered(nerf_ctx *ctx, const float *sigma, const float lo[3], const float step[3], const int32_t dims[3], float iso,
                                  const void *filter, float *vertices, float *normals, size_t cap_vertices, uint32_t *triangles,
                                  size_t cap_triangles, uint64_t *n_vertices, uint64_t *n_triangles, uint64_t *n_components, uint64_t *n_kept);
int nerf_extract_mesh_filtered(nerf_ctx *ctx, int which, const float lo[3], const float step[3], const int32_t dims[3], float iso,
                               const void *filter, float *vertices, float *normals, float *rgb, size_t cap_vertices, uint32_t *triangles,
                               size_t cap_triangles, uint64_t *n_vertices, uint64_t *n_triangles, uint64_t *n_components, uint64_t *n_kept);
int nerf_extract_mesh_filtered_device(nerf_ctx *ctx, int which, const float lo[3], const float step[3], const int32_t dims[3], float iso,
                                      const void *filter, float *d_vertices, float *d_normals, float *d_rgb, size_t cap_vertices,
                                      uint32_t *d_triangles, size_t cap_triangles, uint64_t *n_vertices, uint64_t *n_triangles,
                                      uint64_t *n_components, uint64_t *n_kept, void *stream);

/* ---- S3: render_image (src/lib.rs:474-565) ----------------------------------------------------------------- */
/* rgb_out: crop_h x crop_w x 3 (or ny x nx x 3) linear RGB f32, row-major, index (i*w + j)*3 as image[i*nx+j]
 * (src/lib.rs:552-557).  Unlike the reference (src/lib.rs:491-501) nx, ny need not be multiples of 8. */
int nerf_render_image(nerf_ctx *ctx, const nerf_camera *cam, const nerf_render_opts *opts, float *rgb_out,
                      nerf_stats *stats /* may be NULL */);
/* device output, asynchronous on `stream`; stats != NULL synchronises the stream before returning. */
int nerf_render_image_device(nerf_ctx *ctx, const nerf_camera *cam, const nerf_render_opts *opts, float *d_rgb_out,
                             void *stream, nerf_stats *stats);
/* Colour plus the two other per-pixel maps of a NeRF renderer (nerf-pytorch's rgb_map, depth_map, acc_map).  For each ray, with w_i the
 * exact compositing weights (the T < 1e-4 cut included: zero after it) and t_i its sample positions (the merged fine samples; the coarse
 * ones for coarse_only or when no fine sample is drawn):
 *   opacity = sum_i w_i          in sample order, f32 -- the reference's `acc` (src/lib.rs:185-194); rgb = sum_i w_i c_i + (1 - opacity)
 *   depth   = sum_i (t_i * w_i)  in sample order, f32, separate multiply and add: the expected termination distance along the UNIT ray
 *                                direction (src/lib.rs:371) -- Euclidean distance from the camera centre, not z-depth.  The background
 *                                adds 0: an empty ray has depth 0 and opacity 0; depth / opacity is the depth of the surface hit.
 * SSAA: each map is the box mean of its s x s sub-rays (same order as the colour).  Windows and bands: each map is h x w floats with
 * the colour output's layout.  rgb_out is required, either map may be NULL; with both NULL a call is its counterpart without _aux.
 * The colour is bit-identical whether or not maps are asked for.  Device variant: asynchronous on `stream`, like
 * nerf_render_image_device. */
int nerf_render_image_aux(nerf_ctx *ctx, const nerf_camera *cam, const nerf_render_opts *opts, float *rgb_out,
                          float *depth_out /* h x w or NULL */, float *opacity_out /* h x w or NULL */, nerf_stats *stats);
int nerf_render_image_aux_device(nerf_ctx *ctx, const nerf_camera *cam, const nerf_render_opts *opts, float *d_rgb_out,
                                 float *d_depth_out, float *d_opacity_out, void *stream, nerf_stats *stats);
/* ---- display-ready RGBA8, packed on the device, over any background -------------------------------------------------------------
 * The reference's public display entry point is render_image_rgba(width, height) -> Uint8Array (src/lib.rs:700-726, pixels_to_rgba
 * :582-592): the frame over white, quantised, alpha 255.  These entry points produce those bytes on the device -- 4 bytes per pixel come
 * back instead of 12 -- and add what a compositor needs: another background, or a real alpha channel.
 * For each ray, with w_i the exact compositing weights (zero after the T < 1e-4 cut) and c_i the sample colours:
 *   C = sum_i w_i c_i per channel, A = sum_i w_i: summed in sample order in f32, separate multiply and add -- the sums of nerf_render_image
 *   and the opacity of nerf_render_image_aux.  background B = (B_r, B_g, B_b); NULL = white, the reference.
 *   NERF_ALPHA_OPAQUE         rgb = C + B * (1 - A), multiply and add rounded separately; alpha byte 255.  With B = 1 (or NULL) these are
 *                             the bits of nerf_render_image.
 *   NERF_ALPHA_PREMULTIPLIED  rgb = C (the opaque arithmetic with B = 0, which yields C exactly), alpha = A.  B is ignored.
 *   NERF_ALPHA_STRAIGHT       rgb = C / A where A > 0, else 0 (correctly rounded f32 division, no reciprocal approximation), alpha = A.
 * Every channel, alpha included, is quantised like nerf_quantize_rgb8 (save_ppm, src/lib.rs:573-577): clamp(v, 0, 1) * 255 + 0.5
 * truncated, multiply and add separate; NaN becomes 0 by an explicit test.  Byte for byte the host quantiser.
 * SSAA: the per-ray colour over B, and the per-ray A when the mode needs it, go through the same box filter as nerf_render_image_aux's
 * maps; mode conversion and quantisation happen once per PIXEL on the filtered values (straight alpha divides the mean C by the mean A).
 * Windows, bands, every mlp_dtype, coarse_only, skip_empty, skip_dead, hybrid_sampling and certify_zero behave as in the float entry
 * points; with certify_zero the pack runs on the frame that stands after the retry loop.
 * rgba_out: h x w x 4 bytes, row-major, R,G,B,A per pixel -- the layout nerf_quantize_rgba8 writes.  The f32 frame lives in the
 * context's workspace (grown on demand: a warm call allocates nothing; the single-caller rule above covers it).
 * NERF_ERR_INVALID: alpha_mode outside 0..2, a non-finite background component (finite values outside [0, 1] are allowed: the quantiser
 * clamps), a NULL output. */
enum { NERF_ALPHA_OPAQUE = 0, NERF_ALPHA_PREMULTIPLIED = 1, NERF_ALPHA_STRAIGHT = 2 };
int nerf_render_image_rgba8(nerf_ctx *ctx, const nerf_camera *cam, const nerf_render_opts *opts, const float background[3],
                            int alpha_mode, uint8_t *rgba_out, nerf_stats *stats);
/* device output, asynchronous on `stream` like nerf_render_image_device (stats != NULL and certify_zero synchronise) */
int nerf_render_image_rgba8_device(nerf_ctx *ctx, const nerf_camera *cam, const nerf_render_opts *opts, const float background[3],
                                   int alpha_mode, uint8_t *d_rgba_out, void *stream, nerf_stats *stats);

/* ---- ray batches: render the caller's rays (per-ray origins, directions and bounds) ----------------------------------------------------
 * Every other render entry point takes a nerf_camera, a pinhole camera on a pixel grid.  These take the rays themselves -- the `render_rays`
 * of other NeRF code bases: another lens, rays clipped against the scene box, a picking ray, stereo pairs, a batch of pixels of many poses.
 * Per ray r, every operation in f32, rounded once, never contracted:
 *   DIRECTION  d = dirs[r] when normalize == 0 (the caller promises unit length), else dirs[r] / sqrtf(dx*dx + dy*dy + dz*dz), the sum in
 *              that order, sqrt and division correctly rounded: Vec3::normalize as nerf_stage_ray_dirs applies it.
 *   BOUNDS     [near_r, far_r] = bounds[r] = {near, far}, or [near_, far_] for every ray when bounds is NULL.
 *   COARSE     stratified_samples (src/lib.rs:233-248) over [near_r, far_r] with opts->n_coarse samples, in nerf_stage_stratified's
 *              arithmetic, from Philox stream 0 of (opts->seed, index_r); index_r = rng_index[r], or r when rng_index is NULL.
 *   POINTS     fl(o_r + fl(d * t)) per coordinate; o_r = origins[r], or origins[0] when n_origins == 1.
 *   NETWORKS   the coarse network at the coarse points; compute_weights + sample_importance (nerf_stage_resample) from Philox stream 1 of
 *              the same index, the last interval being far_r - t_last; merge and sort; the fine network at the merged points with d as
 *              view direction; integrate_ray (last interval: far_r - t_last) over `background` (NULL = white; the arithmetic of
 *              nerf_render_image_rgba8's NERF_ALPHA_OPAQUE, which with white is nerf_render_image's).
 *   BRANCHES   those of nerf_render_image: n_fine == 0 or n_coarse < 3 evaluates the fine network on the coarse samples; coarse_only is
 *              honoured; mlp_dtype selects the arithmetic as there (BF16X3 / F16X2: the sampling pass stays in exact f32).
 *   MAPS       depth_out[r], opacity_out[r]: exactly nerf_render_image_aux's sums.  Either may be NULL.
 * CONSEQUENCE  a batch made of a camera's rays -- origins = cam.pos (n_origins = 1), dirs = nerf_stage_ray_dirs of a window, near_ / far_ the
 *              camera's, rng_index = row * nx + col -- carries the bits of nerf_render_image_aux for that window.  The output of ray r
 *              depends on ray r's inputs, opts and the weights alone: permuting a batch (rng_index along with it) permutes its outputs;
 *              n_origins == n_rays with one origin repeated gives the bits of n_origins == 1.
 * LIMITS       n_rays == 0 is a no-op; n_rays <= INT32_MAX.  The batch runs in passes of at most NERF_MAX_RAYS_PER_PASS rays with
 *              rays * samples <= 0x3fffffff, like an image; the limit on samples per ray is the image renders'.  Per-ray origins cost a
 *              workspace of 24 bytes per sample of a pass in the context, grown on demand: a warm call allocates nothing.  (The certified
 *              forms below expand nothing: no such workspace.)
 * REFUSED      the options tied to the pixel grid or to the ray-sequential kernels -- NERF_ERR_INVALID when any of opts->crop_*, ssaa > 1,
 *              band_count > 1, skip_empty, skip_dead, hybrid_sampling is set; opts->certify_zero too, on these entry points: zero
 *              certification of a batch is nerf_render_rays_certified / nerf_render_rays_clipped_certified.  Also NERF_ERR_INVALID:
 *              a NULL origins / dirs / opts / rgb_out, n_origins outside {1, n_rays}, n_coarse <= 0, n_fine < 0, a bad mlp_dtype, near_ /
 *              far_ not finite or far_ <= near_ when bounds is NULL, a non-finite background.  All of this is checked before the context
 *              or the device is needed.
 * PER-RAY CHECKS (host entry point only): a non-finite origin, direction or bound, a zero direction with normalize, far <= near --
 *              NERF_ERR_INVALID, the message names the first offending ray ("ray 17: ...").  nerf_render_rays_device cannot look at the
 *              rays: the outputs of such a ray are unspecified, no other ray is affected.  A ray that misses its volume (far <= near)
 *              is the caller's to leave out.
 * FAILURE      nerf_stats.n_nonfinite_points != 0 fails the call with NERF_ERR_STATE as for an image (the host entry point always reads
 *              the counters, the device one with stats != NULL).  nerf_stats is filled as for an image (n_rays, point counts, ms_*,
 *              n_passes, n_mlp_launches); nerf_kernel_time_query keeps counting image renders only.
 * Host pointers, synchronous. */
int nerf_render_rays(nerf_ctx *ctx, const float *origins /* n_origins x 3 */, size_t n_origins /* 1 or n_rays */,
                     const float *dirs /* n_rays x 3 */, size_t n_rays, int normalize,
                     float near_, float far_, const float *bounds /* n_rays x 2 {near, far}, or NULL: near_, far_ for every ray */,
                     const uint32_t *rng_index /* n_rays, or NULL: ray r draws from index r */,
                     const nerf_render_opts *opts, const float background[3] /* NULL = white */,
                     float *rgb_out /* n_rays x 3 */, float *depth_out /* n_rays or NULL */, float *opacity_out /* n_rays or NULL */,
                     nerf_stats *stats /* may be NULL */);
/* origins, dirs, bounds, rng_index and the outputs are DEVICE pointers; asynchronous on `stream` (stats != NULL synchronises it before
 * returning), except that with n_origins == 1 the origin -- which rides in the MLP kernels' arguments -- is read back first: 12 bytes and one
 * stream synchronisation before the first launch. */
int nerf_render_rays_device(nerf_ctx *ctx, const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize,
                            float near_, float far_, const float *d_bounds, const uint32_t *d_rng_index,
                            const nerf_render_opts *opts, const float background[3],
                            float *d_rgb_out, float *d_depth_out, float *d_opacity_out, void *stream, nerf_stats *stats);
/* nerf_render_rays with zero certification (nerf_render_opts.certify_zero of an image render) inside every pass: the 16-bit pre-filter
 * certifies the samples whose density is 0 and predicts each ray's transmittance cut, the exact kernels evaluate the remaining samples
 * from a device-side list.
 * OUTPUTS      rgb_out, depth_out, opacity_out are those of nerf_render_rays with the same arguments, bit for bit -- shared origin or
 *              per-ray origins, near_ / far_ or per-ray bounds, rng_index, normalize, background, coarse_only, n_fine == 0, several passes.
 * SWITCH       the entry point is the switch: opts->certify_zero must be 0 or 1 and is otherwise not consulted.
 * REFUSED      mlp_dtype NERF_MLP_BF16 ("certify_zero needs mlp_dtype F32, BF16X3 or F16X2 ...", as for an image); skip_empty, skip_dead,
 *              hybrid_sampling, crop_*, ssaa > 1, band_count > 1 with nerf_render_rays' messages.  Every other argument check and per-ray
 *              host check is nerf_render_rays', in the same order, made before the context or the device is needed; a NULL context is
 *              reported last.
 * AUDIT        as for an image: a batch stands only if the audit found no wrong certificate and enough headroom; otherwise the margin is
 *              widened (per context and network) or the list grown and the BATCH IS RENDERED AGAIN, at most 8 times, then NERF_ERR_STATE.
 *              nerf_stats carries n_certify_*, certify_margin / _headroom / _max_error and n_exec_* as for an image.
 * LIMITS       nerf_render_rays'.  Per-ray origins are read by the certified kernels themselves (one origin per list entry / per ray of
 *              the pre-filter): no points are expanded and the 24-byte-per-sample workspace is not needed.  The fused pre-filter
 *              (NERF_CERTIFY_SEQ_PREFILTER=0) knows one origin only: a pass with per-ray origins uses the ray-sequential pre-filter
 *              whatever that setting says.  Normals are not offered.  nerf_kernel_time_query keeps counting image renders only.
 * Host pointers, synchronous. */
int nerf_render_rays_certified(nerf_ctx *ctx, const float *origins /* n_origins x 3 */, size_t n_origins /* 1 or n_rays */,
                               const float *dirs /* n_rays x 3 */, size_t n_rays, int normalize,
                               float near_, float far_, const float *bounds /* n_rays x 2 or NULL */,
                               const uint32_t *rng_index /* n_rays or NULL */,
                               const nerf_render_opts *opts, const float background[3] /* NULL = white */,
                               float *rgb_out /* n_rays x 3 */, float *depth_out /* n_rays or NULL */, float *opacity_out /* n_rays or NULL */,
                               nerf_stats *stats /* may be NULL */);
/* device pointers as for nerf_render_rays_device.  SYNCHRONISES `stream` before returning, with or without stats: the audit that decides
 * whether the batch stands is read on the host (and with n_origins == 1 the origin is read back first, as there). */
int nerf_render_rays_certified_device(nerf_ctx *ctx, const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize,
                                      float near_, float far_, const float *d_bounds, const uint32_t *d_rng_index,
                                      const nerf_render_opts *opts, const float background[3],
                                      float *d_rgb_out, float *d_depth_out, float *d_opacity_out, void *stream, nerf_stats *stats);

/* ---- surface normals: the gradient of sigma at caller points, and one normal per ray of a batch -------------------------------------------
 * The mesh normals above difference sigma over a whole lattice spacing.  These entry points difference the network itself, with a step h
 * the caller chooses, on the device (nerf-rs_amd/csrc/normal_kernels.hip around the f32 sigma-only launch of nerf_density_batch).  All
 * arithmetic is f32; every operation is rounded once and never contracted; division and sqrt are correctly rounded.  A host can restate
 * every output bit for bit from nerf_density_batch and the stage calls (tests/helpers/normal_restatement.py does).
 * GRADIENT   of sigma at a point p with step h (one scalar per call, finite and > 0).  For each axis a in {x, y, z}:
 *              p+ = p with coordinate a replaced by fl(p_a + h), p- = p with coordinate a replaced by fl(p_a - h);
 *              sigma+, sigma- = the bits nerf_density_batch returns at p+ and p- (always the f32 sigma-only kernel);
 *              den = fl(p+_a - p-_a);  g_a = fl(fl(sigma+ - sigma-) / den), and g_a = 0 if den == 0 (h below half an ulp of p_a).
 * RAY NORMAL added to the ray-batch pipeline exactly as nerf_render_rays specifies it, over the samples the final compositing integrates: the
 *            fine pass's n_coarse + n_fine merged samples, or the coarse ones under coarse_only (and in nerf_render_rays' other branches).
 *              w_i = the weight the compositing kernel computes for sample i: the bits of nerf_stage_integrate's w_out on that pass's
 *                    t, sigma (in the render's own mlp_dtype) and far;
 *              x_i = fl(o + fl(d * t_i)) per coordinate, d the direction the networks saw (normalised when normalize != 0);
 *              a sample is LIVE iff w_i > 0 (a NaN weight is not); only live samples are evaluated, every other sample contributes
 *                    nothing whatever its gradient would have been;
 *              G_a = sum over the live i in ascending i of w_i g_a(x_i): acc = fl(acc + fl(w_i * g_a(x_i))), starting from +0;
 *              len = sqrtf(fl(fl(G_x G_x + G_y G_y) + G_z G_z));  n = (-G) / len per component -- towards lower density, the mesh normals'
 *                    convention; n = (0, 0, 0) when len is 0 or not finite, which includes a ray without a live sample.
 *            The network differentiated is the one that was composited (fine, or coarse under coarse_only), always in f32 -- also when
 *            mlp_dtype made the weights in another arithmetic.
 * CONSEQUENCE nerf_render_rays' clauses extend to the normal: a ray's normal depends on that ray's inputs, opts, h and the weights alone;
 *            permuting a batch permutes the normals; shared and repeated origins give the same bits; the pass size changes no bit; and
 *            colour, depth and opacity of a call that also asks for normals are the bits of the same call without them.
 * WORKSPACE  in the context, grown on demand (a warm call allocates nothing): 8 bytes per composited sample of a pass (weights, live
 *            list) + 8 per ray, and 16 bytes per stencil point -- 96 per live sample of a pass.  nerf_density_gradient_batch* runs large n in
 *            internal chunks of at most 2^20 points (NERF_GRADIENT_CHUNK, read by nerf_create, overrides it): its stencil workspace is
 *            bounded by 96 MiB whatever n is, and no bit depends on the chunking.
 * The live count of every pass comes back to the host (8 bytes, one stream synchronisation per pass): it sizes the launches that follow,
 * so nerf_render_rays_normals_device is asynchronous only from its last pass's count on.  A pass without a live sample launches nothing
 * further and writes zero normals.
 * NERF_DEBUG_NORMALS=1 (read by nerf_create): a normals render that fills nerf_stats prints its live share and the device time of its own
 * launches to stderr.  Those launches count into nerf_stats.ms_other and ms_total; n_mlp_launches stays the colour pipeline's. */
/* grad_soa: 3 x n like pts_soa (plane a = dsigma/da).  Host pointers, synchronous; n == 0 is a no-op.  Input domain and largest n: as
 * nerf_density_batch (the stencil points p +- h included).  NERF_ERR_INVALID (checked before the context or the device is needed, "ctx is
 * NULL" last): a bad `which`, h not finite or <= 0, a NULL buffer with n > 0. */
int nerf_density_gradient_batch(nerf_ctx *ctx, int which, const float *pts_soa /*3 x n*/, size_t n, float h, float *grad_soa /*3 x n*/);
/* device pointers, asynchronous on `stream` */
int nerf_density_gradient_batch_device(nerf_ctx *ctx, int which, const float *d_pts_soa, size_t n, float h, float *d_grad_soa, void *stream);
/* nerf_render_rays + normals_out (n_rays x 3).  Every argument, refusal and per-ray check of nerf_render_rays applies unchanged; also
 * NERF_ERR_INVALID, checked with the others before the context or the device is needed: h not finite or <= 0, normals_out NULL. */
int nerf_render_rays_normals(nerf_ctx *ctx, const float *origins /* n_origins x 3 */, size_t n_origins /* 1 or n_rays */,
                             const float *dirs /* n_rays x 3 */, size_t n_rays, int normalize,
                             float near_, float far_, const float *bounds /* n_rays x 2 or NULL */,
                             const uint32_t *rng_index /* n_rays or NULL */,
                             const nerf_render_opts *opts, const float background[3] /* NULL = white */,
                             float *rgb_out /* n_rays x 3 */, float *depth_out /* n_rays or NULL */, float *opacity_out /* n_rays or NULL */,
                             float h, float *normals_out /* n_rays x 3 */, nerf_stats *stats /* may be NULL */);
/* nerf_render_rays_device + d_normals_out (device, n_rays x 3); synchronises once per pass as described above */
int nerf_render_rays_normals_device(nerf_ctx *ctx, const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize,
                                    float near_, float far_, const float *d_bounds, const uint32_t *d_rng_index,
                                    const nerf_render_opts *opts, const float background[3],
                                    float *d_rgb_out, float *d_depth_out, float *d_opacity_out, float h, float *d_normals_out,
                                    void *stream, nerf_stats *stats);

/* ---- quantile depth and point clouds: where a ray meets the surface, and the rays that hit as a coloured point list --------------------------
 * depth_out of the ray batches is the expected termination distance sum_i w_i t_i.  At a silhouette a ray is absorbed partly by the model and
 * partly far behind it, and that number lies in the empty space between the two: unprojected, it gives flying pixels along every edge.  These
 * entry points add the robust depth -- the distance at which the ray has lost a given share of its light; the median depth is the 0.5
 * quantile -- and, on top of it, the export NeRF -> coloured point cloud: one surface point per ray that hit something, with colour and
 * normal (nerf-rs_amd/csrc/surface_kernels.hip behind the compositing launch of every pass).  All arithmetic is f32; every operation is
 * rounded once and never contracted; division is correctly rounded.  A host can restate every output bit for bit from nerf_render_rays,
 * nerf_render_rays_normals and the stage calls (tests/helpers/surface_restatement.py does).
 * QUANTILE DEPTH of a ray, over the samples the final compositing integrates (as for the ray normal: the fine pass's merged samples, or the
 *            coarse ones under coarse_only and in nerf_render_rays' other branches), t_i their positions in ascending i:
 *              w_i   = the weight the compositing kernel computes for sample i: the bits of nerf_stage_integrate's w_out, in the render's own
 *                      mlp_dtype;
 *              cum_0 = +0, cum_i = fl(cum_{i-1} + w_i) in ascending i: exactly the partial sums of the opacity, the last one is the bits of
 *                      opacity_out;
 *              k(q)  = for a quantile q in (0, 1] the smallest i with cum_i >= q; a NaN cum_i compares false, such a sample is never k(q);
 *              depth_q = t_{k(q)}, the sample's own position without interpolation inside the interval; +0 if no such i exists.
 * CONSEQUENCE depth_q is non-zero only if opacity >= q; it does not decrease as q grows, as long as it is non-zero; nerf_render_rays'
 *            clauses extend to it -- a ray's depth_q depends on that ray's inputs, opts and the weights alone, permuting a batch permutes
 *            it, the pass size changes no bit, shared and repeated origins give the same bits -- and colour, depth and opacity of a call
 *            that asks for quantiles are the bits of the same call without them.
 * POINTS     for ONE quantile q and a threshold min_opacity in [0, 1]: ray r is KEPT iff opacity_r >= min_opacity and k(q) exists (a NaN
 *            opacity keeps nothing; a crossing at a position of exactly 0 cannot be told from none and is not kept either).  The kept
 *            rays are written in ascending ray order, over the whole batch and across passes.  Per kept ray:
 *              xyz     = fl(o_r + fl(d * depth_q)) per coordinate, d the direction the networks saw: nerf_render_rays' POINTS formula;
 *              rgb     = C / A per channel; C = sum_i w_i c_i is the colour nerf_render_rays returns over background (0, 0, 0), A the
 *                        opacity: the NERF_ALPHA_STRAIGHT arithmetic.  A > 0 for every kept ray, because cum >= q > 0;
 *              normal  = the bits of nerf_render_rays_normals for that ray with step h; written only when h > 0 is given (normals_out is
 *                        then required); with h == 0 no normals launch is made;
 *              ray     = the index r (uint32), depth = depth_q, opacity = A: three optional arrays.
 *            The compaction is deterministic (prefix sums, no atomics); the running offset between passes stays on the device.
 * CAPACITY   the caller gives the capacity of the output arrays in points; n_rays always suffices.  If more rays are kept than fit, the
 *            first `capacity` points are written and nothing behind them, *n_points carries the full count and the call returns
 *            NERF_ERR_STATE with a message that names both numbers.
 * WORKSPACE  in the context, grown on demand (a warm call allocates nothing): 4 bytes per composited sample of a pass (the weights; shared
 *            with the normals workspace when normals are made too, which then holds them); a points render adds 20 bytes per ray of the
 *            batch (32 with normals) + 4 per ray of a pass.  Per composited sample the walk reads 8 bytes (w, t) and the compositing
 *            launch writes 4 (w).
 * REFUSED    NERF_ERR_INVALID, checked before the context or the device is needed, "ctx is NULL" last: everything nerf_render_rays refuses,
 *            with its messages and in its order (a points call's rgb_out is the points' colour array); then n_q outside 1 ..
 *            NERF_MAX_QUANTILES or a NULL `quantiles`; a quantile that is not finite or lies outside (0, 1]; min_opacity not finite or
 *            outside [0, 1]; h not finite or negative; a missing required output (depth_q_out; xyz_out); normals_out without h > 0, and
 *            h > 0 without normals_out.  The host forms' per-ray checks follow, as for nerf_render_rays.
 * The certified and the clipped forms do not offer quantiles or points. */
#define NERF_MAX_QUANTILES 8
/* nerf_render_rays + `quantiles` (n_q values, HOST memory in both forms) and depth_q_out (n_q x n_rays: one plane of n_rays floats per
 * quantile, in the order given).  Host pointers, synchronous. */
int nerf_render_rays_quantiles(nerf_ctx *ctx, const float *origins /* n_origins x 3 */, size_t n_origins /* 1 or n_rays */,
                               const float *dirs /* n_rays x 3 */, size_t n_rays, int normalize,
                               float near_, float far_, const float *bounds /* n_rays x 2 or NULL */,
                               const uint32_t *rng_index /* n_rays or NULL */,
                               const nerf_render_opts *opts, const float background[3] /* NULL = white */,
                               float *rgb_out /* n_rays x 3 */, float *depth_out /* n_rays or NULL */, float *opacity_out /* n_rays or NULL */,
                               const float *quantiles /* n_q, host */, int n_q, float *depth_q_out /* n_q x n_rays */,
                               nerf_stats *stats /* may be NULL */);
/* nerf_render_rays_device + quantiles (host) and d_depth_q_out (device, n_q x n_rays); asynchronous as nerf_render_rays_device */
int nerf_render_rays_quantiles_device(nerf_ctx *ctx, const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize,
                                      float near_, float far_, const float *d_bounds, const uint32_t *d_rng_index,
                                      const nerf_render_opts *opts, const float background[3],
                                      float *d_rgb_out, float *d_depth_out, float *d_opacity_out,
                                      const float *quantiles, int n_q, float *d_depth_q_out, void *stream, nerf_stats *stats);
/* The point cloud of a batch: nerf_render_rays' ray arguments and opts, then the quantile, the threshold, the normals' step (0: no normals)
 * and the capacity; the outputs hold `capacity` records each, of which the first min(*n_points, capacity) are written.  normals_out,
 * ray_out, depth_out, opacity_out and n_points may be NULL (normals_out goes with h > 0).  Host pointers, synchronous. */
int nerf_render_rays_points(nerf_ctx *ctx, const float *origins /* n_origins x 3 */, size_t n_origins /* 1 or n_rays */,
                            const float *dirs /* n_rays x 3 */, size_t n_rays, int normalize,
                            float near_, float far_, const float *bounds /* n_rays x 2 or NULL */,
                            const uint32_t *rng_index /* n_rays or NULL */, const nerf_render_opts *opts,
                            float quantile, float min_opacity, float h, size_t capacity,
                            float *xyz_out /* capacity x 3 */, float *rgb_out /* capacity x 3 */, float *normals_out /* capacity x 3 or NULL */,
                            uint32_t *ray_out /* capacity or NULL */, float *depth_out /* capacity or NULL */,
                            float *opacity_out /* capacity or NULL */, size_t *n_points /* may be NULL */, nerf_stats *stats /* may be NULL */);
/* device pointers; d_n_points (device, may be NULL) receives the full count as a uint32.  Asynchronous on `stream` like
 * nerf_render_rays_device; the stream is synchronised only when the host n_points or stats is asked for -- without them an overflow of
 * the capacity is visible in *d_n_points alone -- and with h > 0 once per pass, as nerf_render_rays_normals_device does. */
int nerf_render_rays_points_device(nerf_ctx *ctx, const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize,
                                   float near_, float far_, const float *d_bounds, const uint32_t *d_rng_index, const nerf_render_opts *opts,
                                   float quantile, float min_opacity, float h, size_t capacity,
                                   float *d_xyz_out, float *d_rgb_out, float *d_normals_out, uint32_t *d_ray_out, float *d_depth_out,
                                   float *d_opacity_out, size_t *n_points, uint32_t *d_n_points, void *stream, nerf_stats *stats);

/* ---- ray clipping: per-ray [near, far] from an occupancy grid, on the device -----------------------------------------------------------
 * nerf_density_grid packs one occupancy bit per lattice cell; nerf_render_rays takes per-ray bounds.  These entry points are the step
 * between them -- the "occupancy grid -> ray marching bounds" of other NeRF renderers (nerf-rs_amd/csrc/ray_clip_kernels.hip) -- and a render
 * that drops the rays which meet no occupied cell.  This is NOT a certificate: an occupancy grid says nothing about points that were never
 * evaluated (a thin structure between lattice points is lost), so the clip is the caller's explicit choice -- threshold and dilation are
 * the caller's, the clipped bounds are returned, and the render that follows is specified exactly in terms of nerf_render_rays.
 * Every arithmetic step is f32, rounded once, never contracted; division and sqrt are correctly rounded; fl() marks each rounding.
 * max(a, b) = a > b ? a : b and min(a, b) = a < b ? a : b (a NaN in a is dropped, one in b is kept).  A host can restate every output
 * bit for bit (tests/helpers/ray_clip.py does; nerf_debug_clip_rays is the same function the kernel calls, run on the host).
 * GRID      occupancy words in nerf_density_grid's layout: bit b of word w is cell 32 w + b, the linear cell is ix + dims[0] (iy + dims[1] iz);
 *           ceil(N / 32) words, N = dims[0] dims[1] dims[2] <= INT32_MAX.
 * DILATION  nerf_occupancy_dilate: a cell of occ_out is set iff an input cell within Chebyshev distance radius (1..4) of it, inside the
 *           grid, is set; the bits behind cell N - 1 are 0.  n_occupied and bounds (both optional) as nerf_density_grid reports them.
 *           occ_bits and occ_out must not overlap.
 * DIRECTION d = dirs[r], or normalised exactly as nerf_render_rays does (DIRECTION there); [near, far] = bounds[r], or {near_, far_}.
 * CELLS     cell i is the box centred on lattice point i.  Per axis a:
 *             G_lo_a = fl(lo_a - fl(0.5 step_a));  G_hi_a = fl(lo_a + fl(step_a fl((float)dims_a - 0.5)))
 *             plane k: P_a(k) = fl(G_lo_a + fl(step_a (float)k))
 * SLAB      t_in = near, t_out = far; then per axis a = x, y, z:
 *             d_a == 0: the ray is a MISS unless G_lo_a <= o_a < G_hi_a; otherwise the axis constrains nothing
 *             else      inv_a = fl(1 / d_a), ta = fl(fl(G_lo_a - o_a) inv_a), tb = fl(fl(G_hi_a - o_a) inv_a),
 *                       t_in = max(t_in, min(ta, tb)), t_out = min(t_out, max(ta, tb))
 *           a MISS unless t_in < t_out.
 * ENTRY     p_a = fl(o_a + fl(d_a t_in)), q_a = fl(fl(p_a - G_lo_a) / step_a), i_a = clamp(floor(q_a), 0, dims_a - 1); a NaN q_a gives 0
 *           by an explicit test.
 * CROSSINGS s_a = sign(d_a) (0 for a NaN).  s_a != 0: tn_a = fl(fl(P_a(i_a + (s_a > 0)) - o_a) inv_a), always recomputed from the plane's
 *           index, never accumulated; s_a == 0: tn_a = +inf.
 * WALK      t_cur = t_in; at most dims_x + dims_y + dims_z + 3 rounds of
 *             1. a* = the lowest axis with the least tn (tn_y replaces tn_x only if tn_y < tn_x, then tn_z likewise); m = tn_a*;
 *                t_exit = min(m, t_out)
 *             2. if cell i is occupied and t_exit > t_cur: on the first such cell t_first = t_cur; always t_last = t_exit
 *             3. stop if t_out <= m
 *             4. i_a* += s_a*; stop if it leaves [0, dims_a*)
 *             5. t_cur = max(t_cur, m); tn_a* is recomputed
 * RESULT    a ray with such a cell is a HIT: bounds_out[r] = {t_first, t_last} (t_first < t_last), hit_out[r] = 1.  A MISS:
 *           bounds_out[r] = the ray's input {near, far}, hit_out[r] = 0.  n_hit = the sum of the flags.
 * GUARANTEES the walk ends after the bounded number of rounds whatever the floats are; no cell index outside the grid is ever read (the
 *           index is range-checked before the word is loaded); a ray's outputs depend on that ray and the grid alone -- a non-finite
 *           ray has unspecified outputs, for that ray only.  No per-ray host checks.
 * NERF_ERR_INVALID (checked before the context or the device is needed, "ctx is NULL" last): a NULL occ_bits / lo / step / dims, a
 *           dim < 1, a non-finite lo, a step that is not finite or <= 0, N > INT32_MAX; n_rays > INT32_MAX; with n_rays > 0 a NULL
 *           origins / dirs / bounds_out / hit_out; n_origins outside {1, n_rays}; near_ / far_ not finite or far_ <= near_ when bounds is
 *           NULL.  nerf_occupancy_dilate: a NULL occ_bits / dims / occ_out, a dim < 1, N > INT32_MAX, radius outside 1..4, overlapping
 *           occ_bits and occ_out.  n_rays == 0 is a no-op (*n_hit = 0).
 * Host pointers, synchronous; need a context, not a network. */
int nerf_occupancy_dilate(nerf_ctx *ctx, const uint32_t *occ_bits, const int32_t dims[3], int radius, uint32_t *occ_out,
                          uint64_t *n_occupied, int32_t bounds[6]);
/* d_occ_bits / d_occ_out: device pointers; n_occupied / bounds: HOST pointers.  Asynchronous on `stream` unless n_occupied or bounds is
 * given: then the call synchronises the stream before it returns. */
int nerf_occupancy_dilate_device(nerf_ctx *ctx, const uint32_t *d_occ_bits, const int32_t dims[3], int radius, uint32_t *d_occ_out,
                                 uint64_t *n_occupied, int32_t bounds[6], void *stream);
int nerf_clip_rays(nerf_ctx *ctx, const uint32_t *occ_bits, const float lo[3], const float step[3], const int32_t dims[3],
                   const float *origins /* n_origins x 3 */, size_t n_origins /* 1 or n_rays */, const float *dirs /* n_rays x 3 */,
                   size_t n_rays, int normalize, float near_, float far_, const float *bounds /* n_rays x 2 or NULL */,
                   float *bounds_out /* n_rays x 2 */, uint8_t *hit_out /* n_rays */, uint64_t *n_hit /* may be NULL */);
/* occ_bits, origins, dirs, bounds and the two outputs are DEVICE pointers; n_hit is a HOST pointer: asynchronous on `stream` unless it
 * is given -- then the call synchronises the stream before it returns. */
int nerf_clip_rays_device(nerf_ctx *ctx, const uint32_t *d_occ_bits, const float lo[3], const float step[3], const int32_t dims[3],
                          const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize, float near_,
                          float far_, const float *d_bounds, float *d_bounds_out, uint8_t *d_hit_out, uint64_t *n_hit, void *stream);
/* Diagnostic: nerf_clip_rays on the CPU, from the function the kernel calls -- no context, no device.  Same arguments (host pointers) and
 * refusals; n_refused_reads (optional) = cell indices outside the grid that the range check in front of the word load turned away,
 * summed over the rays: 0 unless the walk is wrong.  Host-only. */
int nerf_debug_clip_rays(const uint32_t *occ_bits, const float lo[3], const float step[3], const int32_t dims[3], const float *origins,
                         size_t n_origins, const float *dirs, size_t n_rays, int normalize, float near_, float far_, const float *bounds,
                         float *bounds_out, uint8_t *hit_out, uint64_t *n_hit, uint64_t *n_refused_reads);
/* Clip, drop the misses, render the rest -- all on the device: nerf_clip_rays; the hit rays compacted in ascending ray order (prefix sums:
 * the same bits in every run); nerf_render_rays' pipeline on the compacted batch; the results scattered back.
 *   HIT ray r   rgb / depth / opacity = exactly the bits nerf_render_rays returns for that ray alone with bounds = {t_first, t_last} of
 *               nerf_clip_rays and rng_index = index_r (rng_index[r], or r when rng_index is NULL).
 *   MISSED ray  rgb = background (NULL = white), depth 0, opacity 0: what the compositing arithmetic gives an empty ray.
 * hit_out (n_rays bytes) and n_hit are optional.  The hit count comes back to the host once to size the batch (one stream
 * synchronisation); n_hit == 0 launches nothing after the clip.  Every argument, refusal and per-ray host check of nerf_render_rays
 * applies unchanged, then the grid's refusals above.  nerf_stats is filled as for the compacted batch (n_rays = n_hit; all zero when
 * nothing was hit).  Workspace: at most 72 bytes per ray in the context, grown on demand -- a warm call allocates nothing.  Normals are not
 * offered here.  Host pointers, synchronous. */
int nerf_render_rays_clipped(nerf_ctx *ctx, const uint32_t *occ_bits, const float lo[3], const float step[3], const int32_t dims[3],
                             const float *origins /* n_origins x 3 */, size_t n_origins /* 1 or n_rays */,
                             const float *dirs /* n_rays x 3 */, size_t n_rays, int normalize, float near_, float far_,
                             const float *bounds /* n_rays x 2 or NULL */, const uint32_t *rng_index /* n_rays or NULL */,
                             const nerf_render_opts *opts, const float background[3] /* NULL = white */,
                             float *rgb_out /* n_rays x 3 */, float *depth_out /* n_rays or NULL */, float *opacity_out /* n_rays or NULL */,
                             uint8_t *hit_out /* n_rays or NULL */, uint64_t *n_hit /* may be NULL */, nerf_stats *stats /* may be NULL */);
/* device pointers but for lo, step, dims, opts, background, n_hit and stats; synchronises `stream` once, after the clip, to read the hit
 * count (and the shared origin when n_origins == 1); what follows is asynchronous unless stats != NULL. */
int nerf_render_rays_clipped_device(nerf_ctx *ctx, const uint32_t *d_occ_bits, const float lo[3], const float step[3], const int32_t dims[3],
                                    const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize,
                                    float near_, float far_, const float *d_bounds, const uint32_t *d_rng_index,
                                    const nerf_render_opts *opts, const float background[3],
                                    float *d_rgb_out, float *d_depth_out, float *d_opacity_out, uint8_t *d_hit_out, uint64_t *n_hit,
                                    void *stream, nerf_stats *stats);
/* nerf_render_rays_clipped with the compacted batch rendered by nerf_render_rays_certified's pipeline.  Outputs -- rgb, depth, opacity, hit
 * flags, scatter and n_hit -- are those of nerf_render_rays_clipped with the same arguments, bit for bit.  Arguments and refusals:
 * nerf_render_rays_certified's, then the grid's.  A retry of the audit renders the compacted batch again and does not clip again.
 * nerf_stats as for the compacted batch, with the certify fields.  Host pointers, synchronous. */
int nerf_render_rays_clipped_certified(nerf_ctx *ctx, const uint32_t *occ_bits, const float lo[3], const float step[3], const int32_t dims[3],
                                       const float *origins /* n_origins x 3 */, size_t n_origins /* 1 or n_rays */,
                                       const float *dirs /* n_rays x 3 */, size_t n_rays, int normalize, float near_, float far_,
                                       const float *bounds /* n_rays x 2 or NULL */, const uint32_t *rng_index /* n_rays or NULL */,
                                       const nerf_render_opts *opts, const float background[3] /* NULL = white */,
                                       float *rgb_out /* n_rays x 3 */, float *depth_out /* n_rays or NULL */, float *opacity_out /* n_rays or NULL */,
                                       uint8_t *hit_out /* n_rays or NULL */, uint64_t *n_hit /* may be NULL */, nerf_stats *stats /* may be NULL */);
/* device pointers as for nerf_render_rays_clipped_device.  SYNCHRONISES `stream` after the clip (the hit count) and again before returning,
 * with or without stats: the audit is read on the host. */
int nerf_render_rays_clipped_certified_device(nerf_ctx *ctx, const uint32_t *d_occ_bits, const float lo[3], const float step[3],
                                              const int32_t dims[3], const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays,
                                              int normalize, float near_, float far_, const float *d_bounds, const uint32_t *d_rng_index,
                                              const nerf_render_opts *opts, const float background[3],
                                              float *d_rgb_out, float *d_depth_out, float *d_opacity_out, uint8_t *d_hit_out, uint64_t *n_hit,
                                              void *stream, nerf_stats *stats);

/* ---- S3 over several GPUs of one node (reference: the rayon fan-out over blocks + scatter, src/lib.rs:533-557) ------
 * ctxs[i] is one context per device (nerf_create / nerf_create_multi), each with both networks loaded (weights are
 * replicated).  Context i renders band i of n of the output rows (nerf_render_opts.band_*, set here: the caller's values are
 * ignored) on its own host thread and stream: CONTIGUOUS bands -- first row i*(h/n) + min(i, h%n), h/n + (i < h%n) rows -- when every
 * ray costs the same, single rows dealt out round-robin (band_stripe_rows = 1) when opts->skip_dead, skip_empty or certify_zero make
 * the cost follow the scene; a band is bit-identical to the same rows of a single-context frame (per-pixel counter RNG).  `gather` selects how the bands meet in rgb_out (host, same layout as nerf_render_image):
 *   NERF_GATHER_HOST  each band is copied device -> host into its rows directly (no GPU-to-GPU traffic);
 *   NERF_GATHER_PEER  bands are copied GPU -> GPU over xGMI (hipMemcpyPeerAsync) into a frame on ctxs[0]'s device, then one D2H;
 *   NERF_GATHER_RCCL  ONE ncclAllGather of the bands (RCCL over xGMI; librccl is dlopen'ed on first use): the whole frame
 *                     ends up on every device, then one D2H from ctxs[0].  RCCL refuses two ranks on one device: when contexts
 *                     share a device (single-GPU test boxes) the collective step is rehearsed as device-to-device copies into the
 *                     same equal-slot buffers (same layout, stream ordering and ragged compaction); RCCL proper runs whenever
 *                     the devices are distinct.
 * Synchronous.  per_ctx (n entries) may be NULL.  Several contexts may share a device (tests; no speed-up).  Not re-entrant:
 * calls that share a context -- or, with NERF_GATHER_RCCL, a device (the communicators are cached per device list) -- must not
 * overlap.  Errors of any band are reported on ctxs[0]. */
enum { NERF_GATHER_HOST = 0, NERF_GATHER_PEER = 1, NERF_GATHER_RCCL = 2 };
int nerf_render_image_multi(nerf_ctx *const *ctxs, int n, const nerf_camera *cam, const nerf_render_opts *opts, int gather,
                            float *rgb_out, nerf_stats *per_ctx /* n entries or NULL */);
/* ... with the depth and opacity maps of nerf_render_image_aux (either may be NULL).  Every gather works the same way; the maps ride in
 * the same band slots as the colour (still one all-gather per frame with NERF_GATHER_RCCL). */
int nerf_render_image_multi_aux(nerf_ctx *const *ctxs, int n, const nerf_camera *cam, const nerf_render_opts *opts, int gather,
                                float *rgb_out, float *depth_out, float *opacity_out, nerf_stats *per_ctx);
/* ... as RGBA8 (nerf_render_image_rgba8).  Each context packs its own band; a band is then one 32-bit word per pixel, which the gathers
 * move as integers (one plane: still one all-gather per frame with NERF_GATHER_RCCL).  Same band partition.  Every band's counters are
 * read (nerf_stats.n_nonfinite_points fails the call as in nerf_render_image), whether or not per_ctx is given.  rgba_out must be
 * 4-byte aligned. */
int nerf_render_image_multi_rgba8(nerf_ctx *const *ctxs, int n, const nerf_camera *cam, const nerf_render_opts *opts, int gather,
                                  const float background[3], int alpha_mode, uint8_t *rgba_out, nerf_stats *per_ctx);
/* n contexts, device_ids[i] each (NULL => devices 0..n-1); all-or-nothing. */
int nerf_create_multi(const int *device_ids, int n, nerf_ctx **out /* n entries */);
/* Frees the cached RCCL communicators of NERF_GATHER_RCCL (optional; call after the contexts are idle). */
void nerf_multi_release(void);

/* Rows of band band_index when window_rows rows are split over band_count bands (nerf_render_opts.band_*); host-only.  Negative
 * (NERF_ERR_INVALID) on bad arguments. */
int nerf_band_rows(int window_rows, int band_index, int band_count, int band_stripe_rows);

/* Accumulated device time of the dominant (fine- or coarse-only-MLP) kernel since the last reset: blocks until the
 * recorded events have completed.  Used by bench.py for the roofline line. */
int nerf_kernel_time_query(nerf_ctx *ctx, double *ms_dominant_mlp, uint64_t *points_dominant_mlp, uint32_t *n_launches,
                           int reset);

/* Diagnostic: median in-kernel shader clock (MHz) of the last fine-network MLP launch (NERF_DEBUG_CLOCK=1) or of the last sampling
 * (coarse-network) launch (NERF_DEBUG_CLOCK=2), from s_memtime / s_memrealtime stamps around the tile loop.  Only available when
 * NERF_DEBUG_CLOCK was set to 1 or 2 before nerf_create (NERF_ERR_STATE otherwise, and before the first frame). */
int nerf_debug_shader_clock_mhz(nerf_ctx *ctx, double *mhz);
/* Diagnostic: per persistent workgroup of that launch (of the last sampling launch under NERF_DEBUG_CLOCK=2) {shader cycles, 100 MHz ticks} of
 * its tile loop; out: 2 * n_workgroups values, n_workgroups <= the device's CUs.  The spread of the ticks is the launch's load imbalance. */
int nerf_debug_workgroup_clocks(nerf_ctx *ctx, uint64_t *out, size_t n_workgroups);

/* ---- host helpers around the path ------------------------------------------------------------------------ */
/* camera_from_samples (src/lib.rs:614-645): reads near, far, camera_origin, camera_forward, camera_up, hwf. */
int nerf_camera_from_json(const char *json_path, int width, int height, nerf_camera *out);
int nerf_camera_from_values(float near_, float far_, const float origin[3], const float forward[3],
                            const float up[3], const float hwf[3], int width, int height, nerf_camera *out);
/* Camera from a 3x4 camera-to-world pose (row-major; columns = right, up, -forward, origin -- the layout of
 * "camera_matrix" in tf_reference_samples.json, which the reference reads but never uses).  focal in pixels of a
 * ref_w x ref_h image (hwf); the result equals nerf_camera_from_values(origin, -col2, col1, ...). */
int nerf_camera_from_pose(const float c2w[12], float ref_h, float ref_w, float focal, float near_, float far_, int width,
                          int height, nerf_camera *out);
/* save_ppm (src/lib.rs:567-580): P6, (clamp(v,0,1)*255+0.5) as u8 */
int nerf_save_ppm(const char *path, int width, int height, const float *rgb);
void nerf_quantize_rgb8(const float *rgb, size_t n_pixels, uint8_t *out);
/* pixels_to_rgba (src/lib.rs:582-592; the reference's wasm canvas path): the same quantisation, alpha = 255 */
void nerf_quantize_rgba8(const float *rgb, size_t n_pixels, uint8_t *out /* 4 n_pixels */);
/* One-channel PFM ("Pf"; scale -1 = little-endian; rows bottom-up as the format stores them) of width x height floats given top row
 * first (a depth or opacity map of nerf_render_image_aux).  Host-only. */
int nerf_save_pfm(const char *path, int width, int height, const float *values);
/* PAM ("P7", DEPTH 4, MAXVAL 255, TUPLTYPE RGB_ALPHA): the Netpbm format that holds an alpha channel; rgba = height x width x 4 bytes as
 * nerf_render_image_rgba8 writes them.  Host-only. */
int nerf_save_pam(const char *path, int width, int height, const uint8_t *rgba);

/* Binary little-endian PLY of an indexed triangle mesh: per vertex float x y z [float nx ny nz] [uchar red green blue, quantised like
 * nerf_quantize_rgb8], per face "property list uchar uint vertex_indices" with three indices.  normals / rgb may be NULL; zero vertices or
 * triangles are allowed.  NERF_ERR_INVALID: a missing array, or an index >= n_vertices.  Host-only. */
int nerf_save_ply(const char *path, size_t n_vertices, const float *vertices, const float *normals, const float *rgb, size_t n_triangles,
                  const uint32_t *triangles);

/* ---- stage entry points (device execution, host buffers): the individual functions of render_block, exposed so
 * that a host that owns ray setup can call them and so that each stage has its own parity test ------------- */
/* Camera::get_ray_dir (src/lib.rs:213-231) for the rectangle [y0,y0+h) x [x0,x0+w); normalize != 0 applies
 * Vec3::normalize (src/lib.rs:371).  out: h x w x 3 */
int nerf_stage_ray_dirs(nerf_ctx *ctx, const nerf_camera *cam, int x0, int y0, int w, int h, int normalize,
                        float *dirs_out);
/* stratified_samples (src/lib.rs:233-248) for the same rectangle; out: h x w x count */
int nerf_stage_stratified(nerf_ctx *ctx, const nerf_camera *cam, int x0, int y0, int w, int h, int count,
                          uint64_t seed, float *t_out);
/* compute_weights + sample_importance + merge/sort (src/lib.rs:250-351, 414-420) for n_rays rays.
 * u (n_rays x nf) may be NULL => Philox stream 1 of pixel_index[ray].  Outputs may be NULL except t_fine. */
int nerf_stage_resample(nerf_ctx *ctx, size_t n_rays, int nc, int nf, float far_, uint64_t seed,
                        const uint32_t *pixel_index, const float *t_coarse, const float *sigma_coarse, const float *u,
                        float *w_out, float *cdf_out, float *t_new_out, float *t_fine_out);
/* hybrid_sampling's per-ray decision (nerf_render_opts.hybrid_sampling), exposed so that its promise can be tested directly: the same
 * kernel, inputs and RNG as nerf_stage_resample; flags_out[r] = 1 iff ray r would be redone in f32 (a draw predicted to move by more
 * than tau in t under the split arithmetics' density error, or a transmittance within 0.1 % of the cut).  tau = 0 selects the
 * context's threshold (1e-5).  t_new_out (n_rays x nf, the unsorted draws) optional. */
int nerf_stage_hybrid_flags(nerf_ctx *ctx, size_t n_rays, int nc, int nf, float far_, uint64_t seed,
                            const uint32_t *pixel_index, const float *t_coarse, const float *sigma_coarse, const float *u,
                            float tau, uint8_t *flags_out, float *t_new_out);
/* The depth-order table of an image pass (debug / tests): the kernel that runs in front of the fine f32 launch of a pass of `rows` rows of
 * rays_per_row rays with samples_per_ray samples each, on the caller's t (rows x rays_per_row x samples_per_ray, any bits).  The first
 * (rows / 4) * 4 rows are cut in 8 x 4 pixel blocks, row-major; entry q of block b (table_out[32 samples_per_ray b + q]) is the slot
 * ray * samples_per_ray + sample of the point at position q of the block's ascending order by (uint32 bits of t, ray-in-block row-major,
 * sample).  The fine kernel's workgroup tile T evaluates entries 128 T .. 128 T + 127, wave w entries 128 T + 32 w ...  Needs
 * rays_per_row % 8 == 0, rows >= 4, samples_per_ray % 32 == 0 and <= 512 (NERF_ERR_INVALID otherwise: such a pass keeps the static
 * mapping of nerf_debug_wave_tiling, as do skip_empty renders and contexts created under NERF_DEPTH_ORDER=0 or NERF_WAVE_TILING=0).
 * table_out: (rows / 4) * 4 * rays_per_row * samples_per_ray entries. */
int nerf_stage_depth_order(nerf_ctx *ctx, int rows, int rays_per_row, int samples_per_ray, const float *t, uint32_t *table_out);
/* The same kernel's word per pixel block (debug / tests; what the fine cut relies on, NERF_FINE_CUT): flags_out[b] = 1 iff in every one of
 * block b's 32 rows the keys (uint32 bits of t) << 32 | ray-in-block * samples_per_ray + sample ascend with the sample index -- a ray's
 * samples then stand in the table in index order; equal t are in order by the key's low word -- and 0 otherwise (such a block is walked to
 * its end).  flags_out: (rows / 4) * (rays_per_row / 8) words.  The same conditions as nerf_stage_depth_order. */
int nerf_stage_depth_order_flags(nerf_ctx *ctx, int rows, int rays_per_row, int samples_per_ray, const float *t, uint32_t *flags_out);
/* integrate_ray (src/lib.rs:176-195); w_out (n_rays x n) optional */
int nerf_stage_integrate(nerf_ctx *ctx, size_t n_rays, int n, float far_, const float *rgb_aos, const float *sigma,
                         const float *t, float *rgb_out, float *w_out);
/* integrate_ray + the RGBA8 pack (nerf_render_image_rgba8's arithmetic for n_rays rays of n > 0 samples each, one "pixel" per ray);
 * rgba_out: n_rays x 4 bytes */
int nerf_stage_integrate_rgba8(nerf_ctx *ctx, size_t n_rays, int n, float far_, const float *rgb_aos, const float *sigma,
                               const float *t, const float background[3], int alpha_mode, uint8_t *rgba_out);
/* The quantile walk ("quantile depth and point clouds") over n_rays rays of n > 0 samples: w, t n_rays x n; depth_q_out n_q x n_rays.
 * Argument errors are reported before the context is looked at. */
int nerf_stage_ray_quantiles(nerf_ctx *ctx, size_t n_rays, int n, const float *w, const float *t, const float *quantiles, int n_q,
                             float *depth_q_out);
/* The compaction of the kept rays (opacity >= min_opacity and depth_q != 0) into point records, in one pass: origins n_origins x 3
 * (n_origins 1 or n_rays), dirs as the networks saw them, premultiplied_rgb the colour C over black, normals n_rays x 3 or NULL (with
 * normals_out).  Every output array is returned as the device held it: `capacity` records, then NERF_STAGE_GUARD_WORDS (64) words, every
 * word 0xFFFFFFFF before the launches.  *n_points: the full count; NERF_ERR_STATE if it exceeds the capacity.  Argument errors are
 * reported before the context is looked at. */
int nerf_stage_gather_points(nerf_ctx *ctx, size_t n_rays, const float *origins, size_t n_origins, const float *dirs, const float *depth_q,
                             const float *premultiplied_rgb, const float *opacity, const float *normals, float min_opacity, size_t capacity,
                             float *xyz_out, float *rgb_out, float *normals_out, uint32_t *ray_out, float *depth_out, float *opacity_out,
                             size_t *n_points);

/* ---- the device pieces of nerf_render_opts.certify_zero, one launch each on caller data (the launches a certified render makes).
 * Argument errors are reported before the context is looked at.  A list or aux buffer is returned as the device held it, between
 * guards: NERF_STAGE_GUARD_WORDS words, the entries, NERF_STAGE_GUARD_WORDS words, every one of them 0xFFFFFFFF before the launch. */
#define NERF_STAGE_GUARD_WORDS 64
/* The plan kernel over n_rays rays of spr samples.  pre (in/out, n_rays x spr): the pre-filter's density pre-activations; afterwards 0, or
 * -1 on an uncertain sample at or behind the ray's predicted cut jstar_out[ray] (spr: no cut) = the first sample with optical depth
 * sum max(pre, 0) max(delta, 0) in front of it > depth_limit.  A sample is certified iff -3e38 <= pre < -margin.  In front of the cut the
 * uncertain samples are listed, and of the certified ones those with ((index ^ audit_salt) * 0x9E3779B1 mod 2^32) >> 7 & mask == 0, mask =
 * audit_mask_near where pre > -2 margin, else audit_mask -- with bit 31 set and a record {index, bits of pre} in aux (at most 256 per
 * rays_per_wave_out consecutive rays; the others are certified unaudited).  back_part != 0: audited certificates and listed samples with
 * pre < -zero_threshold go to the back part (entry k at list_capacity - 1 - k).  counts_out[3] = {front, back, aux} entries WANTED:
 * beyond a capacity they are counted, not stored, and an audit without an aux record loses its flag.
 * list_out: list_capacity + 2 NERF_STAGE_GUARD_WORDS words; aux_out: 2 aux_capacity + 2 NERF_STAGE_GUARD_WORDS words. */
int nerf_stage_cert_plan(nerf_ctx *ctx, size_t n_rays, int spr, float far_, float margin, float depth_limit, uint32_t audit_mask,
                         uint32_t audit_mask_near, uint32_t audit_salt, int back_part, float zero_threshold, uint32_t list_capacity,
                         uint32_t aux_capacity, const float *t, float *pre, int32_t *jstar_out, uint32_t *list_out,
                         uint32_t *counts_out, uint32_t *aux_out, int32_t *rays_per_wave_out);
/* The verify kernel: compute_weights' transmittance recurrence (src/lib.rs:261-280) over samples [0, jstar[ray]) of sigma (in/out: exact
 * densities, -1 = marked).  Every mark at or behind jstar is cleared; if T did not fall below 1e-4 inside the prefix the marked samples are
 * appended to the list at *count (in/out; counted beyond list_capacity, not stored) and *fallback_rays (in/out) += 1.  A ray with
 * jstar = spr is left alone.  list_out: list_capacity + 2 NERF_STAGE_GUARD_WORDS words. */
int nerf_stage_cert_verify(nerf_ctx *ctx, size_t n_rays, int spr, float far_, uint32_t list_capacity, const float *t, const int32_t *jstar,
                           float *sigma, uint32_t *list_out, uint32_t *count, uint32_t *fallback_rays);
/* The audit kernel over the first min(aux_count, aux_capacity) records {sample, bits of the pre-filter's pre-activation} of aux; sigma
 * (in/out, n_sigma floats) holds the exact RAW pre-activation v of each.  audit (in/out, 4 words): [0] += records, [1] += those with v > 0 or
 * NaN, [2] = max(itself, 0x7f800000 - bits(-v)) over v <= 0, [3] = max(itself, bits |pre - v|) over finite differences; sigma = 0 at every
 * record unless v > 0. */
int nerf_stage_cert_audit(nerf_ctx *ctx, const uint32_t *aux, uint32_t aux_count, uint32_t aux_capacity, size_t n_sigma, float *sigma,
                          uint32_t *audit);
/* The ray-sequential 16-bit pre-filter (f16 != 0: f16 operands, else bf16) of network `which` over n_rays rays from one origin: dirs
 * n_rays x 3 (unit), t n_rays x spr.  pre_out: the raw density pre-activations; a ray is retired after the 32-sample chunk in which its
 * transmittance (from max(pre, 0)) fell below cut_T -- its later samples read 0xFFFFFFFF, "not evaluated"; cut_T = 0 never retires a ray.
 * *nonfinite_tiles: wave tiles of the f16 form with a non-finite pre-activation.  NERF_ERR_STATE: f16 asked for and the network has no
 * f16 stream (a weight beyond the f16 range). */
int nerf_stage_prefilter(nerf_ctx *ctx, int which, int f16, const float origin[3], const float *dirs, const float *t, size_t n_rays,
                         int spr, float far_, float cut_T, float *pre_out, uint32_t *nonfinite_tiles);
/* The same with one origin per ray (origins: n_rays x 3), as a certified ray batch with per-ray origins launches it: row r of pre_out
 * carries the bits nerf_stage_prefilter returns for ray r alone with origin = origins[r]. */
int nerf_stage_prefilter_rays(nerf_ctx *ctx, int which, int f16, const float *origins, const float *dirs, const float *t, size_t n_rays,
                              int spr, float far_, float cut_T, float *pre_out, uint32_t *nonfinite_tiles);

/* "" for the product build.  Tuning / timing-only builds (make variant: some of their switches make results WRONG on purpose)
 * report "NAME: compile definitions"; a host should refuse such a library outside experiments (the Python loader does). */
const char *nerf_build_variant(void);
/* ABI version (currently 5): bumped on any signature or struct change (2: multi-GPU entry points, skip_dead, n_exec_* statistics; 3: nerf_stats.
 * n_nonfinite_points, nerf_check_network_blob, nerf_stage_hybrid_flags, nerf_build_variant; 4: nerf_render_opts.certify_zero; 5: nerf_stats.
 * n_certify_* / certify_margin / certify_headroom / certify_max_error, renders fail on n_nonfinite_points != 0,
 * nerf_render_opts.band_*, nerf_band_rows, nerf_debug_certify_policy; additive: nerf_render_image_aux, nerf_render_image_aux_device,
 * nerf_render_image_multi_aux, nerf_save_pfm, nerf_render_image_rgba8, nerf_render_image_rgba8_device, nerf_render_image_multi_rgba8,
 * nerf_stage_integrate_rgba8, nerf_save_pam, NERF_ALPHA_*, nerf_density_batch, nerf_density_batch_device, nerf_density_grid,
 * nerf_density_grid_device, nerf_isosurface_grid, nerf_extract_mesh, nerf_extract_mesh_device, nerf_save_ply, nerf_component_filter,
 * nerf_component, nerf_lattice_components, nerf_lattice_components_device, nerf_isosurface_grid_filtered, nerf_extract_mesh_filtered,
 * nerf_extract_mesh_filtered_device, nerf_render_rays, nerf_render_rays_device, nerf_density_gradient_batch,
 * nerf_density_gradient_batch_device, nerf_render_rays_normals, nerf_render_rays_normals_device, nerf_stage_cert_plan,
 * nerf_stage_cert_verify, nerf_stage_cert_audit, nerf_stage_prefilter, nerf_occupancy_dilate, nerf_occupancy_dilate_device, nerf_clip_rays,
 * nerf_clip_rays_device, nerf_debug_clip_rays, nerf_render_rays_clipped, nerf_render_rays_clipped_device, nerf_render_rays_certified,
 * nerf_render_rays_certified_device, nerf_render_rays_clipped_certified, nerf_render_rays_clipped_certified_device,
 * nerf_stage_prefilter_rays, nerf_render_rays_quantiles, nerf_render_rays_quantiles_device, nerf_render_rays_points,
 * nerf_render_rays_points_device, nerf_stage_ray_quantiles, nerf_stage_gather_points, NERF_MAX_QUANTILES). */
int nerf_abi_version(void);
/* sizeof(nerf_camera), sizeof(nerf_render_opts), sizeof(nerf_stats) as this library was built: lets a binding written in
 * another language (the Rust `-sys` crate, ctypes) check its struct mirrors at start-up. */
void nerf_abi_struct_sizes(size_t *camera, size_t *render_opts, size_t *stats);

#ifdef __cplusplus
}
#endif
#endif

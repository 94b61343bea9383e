// nerf_internal.h -- the context and what the host files of the device half of the ABI need from each other: nerf_context.cpp (context,
// device memory, events), nerf_networks.cpp (weight upload, MLP launcher), nerf_render.cpp (pass pipeline, render entry points),
// nerf_queries.cpp (point / grid / mesh / stage entry points) and nerf_multi.cpp (multi-GPU fan-out).  Internal to libnerf_mi355x.so;
// nothing here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "../../include/nerf_mi355x.h"
#include "stage_layout.h"

struct MlpArgs;    // mlp_kernel.h
struct SeqArgs;
struct ColourArgs;
struct RayGenArgs; // sampling_kernels.h

namespace nerfint {

// certify_zero: a sample is a certain zero iff its 16-bit (pre-filter) density pre-activation is below -margin.  Floors per network WITH THE bf16
// PRE-FILTER (networks beyond the f16 range), set by the statistic
// the audit watches -- the largest |bf16 - exact| on an audited certificate, which widens the margin above half of it: lego coarse 0.15-0.20
// (a fifth of 1.0), fine 0.99-1.24 (a third to 0.41 of 3.0; at round 3's fine margin of 2 it would trip the rule on most frames).  Round 3's
// fuzz without an audit: coarse 0.5 / fine 1.0 never differed in 10 031 frames, 0.25 / 0.5 did in 1 % of them.  What the floors cost in work
// (C3 frame, exact evaluations: tools/sweep_certify_margins.py): coarse 0.5 -> 8.2 %, 1.0 -> 12.2 %, 1.5 -> 18.6 % of the samples; fine 2 -> 18.8 %,
// 3 -> 20.7 %, 4 -> 23.3 %.
constexpr float kCertMarginCoarse = 1.0f, kCertMarginFine = 3.0f;
// The same floors when the pre-filter runs in f16 (mlp_kernel_f16v2.hip; the default wherever the network's weights fit the f16 range): its
// pre-activations are 8 x closer to the exact ones (numpy emulation on lego rays: largest |f16 - f32| on true zeros 0.048 coarse / 0.113 fine
// against bf16's 0.20 / 0.87), so the margins can be tighter by about that factor with the same distance between floor and largest audited error
// (audited errors on lego: 0.03-0.055 / 0.12-0.17; floor sweep: profiles/r04_certify_f16_prefilter_margin_sweep.log -- fine 0.3 trips the half-margin rule).
constexpr float kCertMarginCoarseF16 = 0.25f, kCertMarginFineF16 = 0.5f;

// what a pair of events brackets (finish_stats sorts the times by it)
enum EvKind {
    EV_COARSE_MLP = 0,   // the sampling pass's network launch
    EV_IMAGE_COLOUR = 1, // the colour-producing network launch of an image render: the dominant kernel (nerf_kernel_time_query)
    EV_OTHER = 2,
    EV_COLOUR_SIDE = 4,  // colour head of skip_dead; certify_zero's launches around the list kernel of the colour-producing network
    EV_BATCH_COLOUR = 5, // the colour-producing network launch of a ray batch (never in `dominant`)
    EV_NORMAL_SIGMA = 6, // the sigma-only stencil launch of a normals render
    EV_NORMAL_SMALL = 7, // its small kernels
};

struct EvPair {
    hipEvent_t a, b;
    EvKind kind;
    bool dominant; // owned by ctx->dominant (handed over by a finished image render: recycle_dominant returns it to the pool); else by
                   // ctx->last_render (recycle_render does)
    uint64_t points;
};

// A device buffer of the context that grows on demand and is freed with it: nerf_destroy walks nerf_ctx::buf.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0; // capacity
    int ensure(nerf_ctx *c, size_t need); // grows only; a regrow synchronises the device and frees the old buffer first
    int release(nerf_ctx *c);             // synchronises the device and frees
};

// A network on the device: every arithmetic's weight stream and the two small blocks, each an owned buffer (nerf_networks.cpp upload_network
// fills them, nerf_destroy walks them).  A released stream = that arithmetic is unavailable for this network (a weight exceeds the f16 range).
enum NetBuf {
    NET_F32,       // the f32 kernels' stream: the FOLDED image (mlp_layout.h kChunksFullFolded; host_util.h fold_network)
    NET_SMALL,     // small block of the packed image: the 16-bit arithmetics, which run the unfolded head
    NET_SMALL_F32, // small block of the folded image (viewdirs bias = b'): the f32 kernels
    NET_BF16V2,    // bf16 pieces in output-tile-major order (mlp_kernel_bf16v2.hip)
    NET_X3,        // three bf16 parts per weight (mlp_kernel_bf16x3.hip)
    NET_X2,        // two f16 parts per weight (mlp_kernel_f16x2.hip)
    NET_F16V2,     // one f16 per weight in NET_BF16V2's order (mlp_kernel_f16v2.hip: certify_zero's pre-filter)
    NET_BUF_COUNT
};
struct DevNet {
    DevBuf buf[NET_BUF_COUNT];
    const float *at(NetBuf id) const { return (const float *)buf[id].p; } // as MlpArgs / SeqArgs carry every stream
    bool loaded = false;    // set once, after every stream of a load is on the device; a load that fails part-way leaves it false
    bool zero_skip = false; // the f32 kernels may skip all-zero ReLU k-steps: the context allows it and every parameter of the folded image is finite
};

enum BufId {
    // pass workspace: ensure_workspace grows the seven together (BUF_RGBC only once a coarse_only render asks for it)
    BUF_DIRS, BUF_TC, BUF_SC, BUF_RGBC, BUF_TF, BUF_SF, BUF_RGBF,
    BUF_RAYFB,      // SSAA ray framebuffer
    BUF_RAYAUX,     // SSAA ray-level depth + opacity maps (nerf_render_image_aux)
    BUF_OUT,        // staging of the host-pointer render entry points (and of nerf_render_image_multi's bands)
    BUF_PACK,       // RGBA8 renders: the f32 frame [+ opacity plane] the pack kernel reads (a host-pointer call stages the packed words in BUF_OUT)
    BUF_BATCH,      // ray batches with per-ray origins / bounds: per pass {far per ray, points 3 x n SoA, directions n x 3 AoS}
    BUF_SCRATCH,    // staging of forward_batch, the queries and the stage calls; an extracted mesh
    BUF_MESH,       // isosurface extraction (isosurface_kernels.h): the per-lattice-point workspace
    BUF_COMP,       // lattice components (components_kernels.h): labels, sizes / keep flags; only when a filter or a component query is asked for
    BUF_NORMAL,     // surface normals (normal_kernels.h): per pass {weights, live list: 4 B per sample each; count, base per ray; block sums; total}
    BUF_STENCIL,    // per stencil point 16 B {3 coordinates, sigma}; also serves nerf_density_gradient_batch, chunk by chunk
    BUF_SURFACE,    // quantile depths and point clouds (surface_kernels.h): per pass the weights (4 B per sample, unless a normals workspace holds them) and the
                    // kept-ray list; a points render: per ray of the batch colour, opacity, quantile depth [, normal]; block sums; the running count
    BUF_CLIP,       // ray clipping (ray_clip_kernels.h): per ray of a batch the clipped bounds, hit flag and compacted copies of a clipped render; block sums
    BUF_SEQ,        // skip_dead: one SeqCounters per MLP launch of a render
    BUF_H8,         // ... the compacted trunk outputs of the live samples (reserve_seq gives a much too large one back)
    BUF_SLOT_POINT, // ... and their sample indices
    BUF_FLAG_LIST,  // hybrid sampling: rays whose coarse pass is redone in f32
    BUF_POINT_LIST, // certify_zero: samples the exact kernel evaluates (one list, reused by every launch)
    BUF_CERT,       // ... one CertCounters per (pass, network)
    BUF_JSTAR,      // ... per ray of a pass: first sample behind the predicted cut
    BUF_CERT_AUX,   // ... {sample, 16-bit (pre-filter) pre-activation} of the audited certificates of a launch
    BUF_ORDER,      // depth-order table of the pass under way: one slot per point of its ordered region
    BUF_ORDER_FLAGS, // ... and one word per pixel block of it: 1 = every ray's samples stand in the table in index order (fine cut; DepthOrderArgs.flags)
    // fixed size, allocated by nerf_create (NULL where that failed or the diagnostic is off)
    BUF_SKIP,       // u64: skipped 128-point tiles (skip_empty; NERF_DEBUG_EMPTY_TILES: of the voted launch under way)
    BUF_NONFINITE,  // u32: non-finite density pre-activations (Arith::counts_range)
    BUF_CLOCK,      // NERF_DEBUG_CLOCK: per workgroup {cycles, 100 MHz ticks} of the last fine-MLP launch
    BUF_ZSKIP,      // NERF_DEBUG_ZSKIP=1: {executed, total} ReLU k-steps of the f32 launch under way
    BUF_CUT,        // coarse and fine cut (MlpArgs.cut_counters; their launches are ordered on the stream): u32 unit counter of the cut launch under way, u32 unused, u64 tiles not evaluated (NERF_DEBUG_COARSE_CUT, NERF_DEBUG_FINE_CUT)
    BUF_COUNT
};

// The counters of one (pass, network) of a certify_zero render (nerf_render.cpp cert_pass, sampling_kernels.hip k_cert_*).  Device code
// receives pointers to single words; launch_cert_audit receives &audited and writes the four words from there.
struct CertCounters {
    uint32_t list1_len, list2_len;                            // wanted lengths of the two sample lists (entries beyond the capacity are counted, not stored)
    uint32_t audited, violations, headroom_code, max_err_bits; // the audit
    uint32_t fallback_rays;                                   // rays whose predicted cut the exact transmittance did not confirm
    uint32_t aux_count;                                       // audit records
    uint32_t pf_ray_head;                                     // the pre-filter's ray queue
    uint32_t list1_back_len;                                  // list 1's back part (probable zeros, audited certificates)
    unsigned long long pf_samples;                            // samples the pre-filter evaluated
    uint32_t range_left;                                      // f16 pre-filter: wave tiles in which an activation left the f16 range
    uint32_t unused[3];
};
static_assert(sizeof(CertCounters) == 64 && offsetof(CertCounters, audited) == 8 && offsetof(CertCounters, max_err_bits) == 20 &&
              offsetof(CertCounters, pf_samples) == 40 && offsetof(CertCounters, range_left) == 48, "CertCounters: sixteen words, the u64 at words 10 and 11");

// The counters of one MLP launch of a skip_dead render (per pass: coarse, fine, hybrid f32 redo of the coarse pass).
struct SeqCounters {
    uint32_t ray_head;            // ray queue
    uint32_t live_count;          // live samples; the hybrid redo's slot: flagged rays
    unsigned long long evaluated; // samples the trunk launch evaluated
};
static_assert(sizeof(SeqCounters) == 16 && offsetof(SeqCounters, evaluated) == 8, "SeqCounters: four words");

} // namespace nerfint

struct nerf_ctx {
    int device = 0;
    int n_cus = 0;
    std::string arch;
    std::string err;
    hipStream_t stream = nullptr; // used by the host-pointer entry points
    nerfint::DevNet net[2];
    size_t ws_rays = 0, ws_nc = 0, ws_m = 0; // what the pass workspace holds
    nerfint::DevBuf buf[nerfint::BUF_COUNT];
    template <class T = float>
    T *dev(nerfint::BufId id) const { return (T *)buf[id].p; } // the buffer, typed
    size_t gradient_chunk = (size_t)1 << 20;             // points per internal chunk of nerf_density_gradient_batch (NERF_GRADIENT_CHUNK)
    bool debug_normals = false;                          // NERF_DEBUG_NORMALS=1: a normals render with stats prints its live share and kernel times
    uint64_t normal_live = 0, normal_samples = 0;        // of the last normals render: live / composited samples
    float cert_margin[2] = {nerfint::kCertMarginCoarse, nerfint::kCertMarginFine}; // widened by render_device when an audit fails; reset at load
    float cert_margin_floor[2] = {nerfint::kCertMarginCoarse, nerfint::kCertMarginFine};
    float cert_margin_floor_f16[2] = {nerfint::kCertMarginCoarseF16, nerfint::kCertMarginFineF16};
    bool cert_prefilter_f16[2] = {false, false}; // per network: the pre-filter runs in f16 (set at load when the weights fit; cleared for good when an activation left the f16 range)
    bool cert_allow_f16 = true;
    float cert_depth_limit = 9.6f;        // predicted cut: bf16 optical depth > 9.6 (the exact cut is at T < 1e-4 = depth 9.21; nothing but work depends on it:
                                          // lego frame 0 rays fall back at 9.5, 25 at 9.35, 1132 of 640 000 at 9.25 -- tools/sweep_certify.py)
    unsigned cert_audit_mask = 127;       // one certified sample in 128 is audited ...
    unsigned cert_audit_mask_near = 15;   // ... and one in 16 of those certified by less than twice the margin: the same number of audits as a flat 1 in 64
                                          // on the lego frame, four times as many where a certificate is at risk
    bool cert_zero_tiles = true;          // probable zeros + audited certificates in the list's back part, evaluated with skip_empty
    float cert_zero_frac = 0.1f;          // "probably zero": pre-filter pre-activation below -margin x this (C3 frame: 1/2 -> 334.6 ms, 1/3 -> 333.1, 0.1 -> 330.5, 0.02 -> 331.0: tools/sweep_certify_zero_frac.py)
    bool cert_seq_prefilter = true;       // 16-bit pre-filter ray-sequential with its own predicted cut (false: the fused 16-bit kernel over all samples)
    double cert_list_frac = 0.5;          // list capacity as a fraction of a pass's samples: what earlier frames needed + 25 %
    float hybrid_tau = 1e-5f;                                        // a draw predicted to move by more than this (in t) flags its ray
    size_t max_export_bytes = (size_t)16 << 30; // budget of BUF_H8: bounds the rays per pass of skip_dead in a SPLIT arithmetic (NERF_MAX_EXPORT_BYTES);
                                                // 16 GiB = 8 passes per 800x800 frame, 1.4 % slower than one pass of 128 GiB
    bool clock_valid = false;
    bool clock_coarse = false;             // NERF_DEBUG_CLOCK=2: the clocks are those of the last sampling (coarse) launch
    bool zero_step_skip = true;            // NERF_ZERO_STEP_SKIP=0 at nerf_create: the f32 kernels execute every k-step (networks loaded afterwards)
    bool ray_grouping = true;              // NERF_RAY_GROUPING=0 at nerf_create: ray-mode f32 launches keep 128 consecutive samples per workgroup tile (mlp_layout.h)
    bool wave_tiling = true;               // NERF_WAVE_TILING=0 at nerf_create: a wave of a ray-mode f32 launch keeps 32 consecutive samples of one ray (mlp_layout.h)
    bool depth_order = true;               // NERF_DEPTH_ORDER=0 at nerf_create: the fine launch of an image pass keeps the static wave tiling (mlp_layout.h DepthOrder)
    bool tile_rotation = true;             // NERF_TILE_ROTATION=0 at nerf_create: round k's tile of persistent workgroup c of the f32 fused kernel is k G + c (mlp_layout.h rotated_tile)
    bool empty_tile_vote = true;           // NERF_EMPTY_TILE_VOTE=0 at nerf_create (or NERF_DEBUG_ZSKIP=1: the k-step diagnostic describes the dense colour head): full ray-mode launches of a plain render evaluate the colour head of all-empty tiles too (MlpArgs.empty_vote)
    bool debug_empty_tiles = false;        // NERF_DEBUG_EMPTY_TILES=1 at nerf_create: every voted launch counts its skipped tiles in BUF_SKIP and prints them (synchronises: a diagnostic)
    // A cut launch hands out whole pixel blocks (spr / 4 tiles each), so a launch with few blocks per workgroup loses parallelism: 128 blocks keep
    // 128 of 256 workgroups busy for 16 tiles each where the static walk gives each of the 256 eight.  With B blocks on G workgroups the queue ends
    // at most one block behind the mean, a share G / B of the launch: from 16 blocks per workgroup on that is below 1 / 16, whatever the scene cuts.
    static constexpr int kCutMinBlocksPerWorkgroup = 16;
    int coarse_cut = 1;                    // 2 (NERF_COARSE_CUT=2): every qualifying launch is cut, however few blocks it has (tests, diagnostics); 1: launches of at least kCutMinBlocksPerWorkgroup blocks per workgroup; NERF_COARSE_CUT=0 at nerf_create (or NERF_DEBUG_ZSKIP=1: the k-step totals describe every sample): the f32 sampling launch of a plain render evaluates the samples behind every ray's T < 1e-4 cut too (MlpArgs.ray_cut)
    bool debug_coarse_cut = false;         // NERF_DEBUG_COARSE_CUT=1 at nerf_create: every cut launch counts the tiles it did not evaluate in BUF_CUT and prints them (synchronises: a diagnostic)
    // The fine cut hands out whole blocks too, and a fine block is three times as long (spr / 4 = 48 tiles at 64 + 128, 7.5 ms of a 590 ms launch):
    // the queue ends at most one block behind the mean, a share G / B of the launch, and what the cut can win on the lego frame is about 5 %
    // of the launch (the tiles behind the last ray's cut, profiles/finecut_cpu_model.txt).  From 48 blocks per workgroup on the worst case of
    // the tail is 2.1 %, its mean half of that: below the gain.  The bench frame has 78 per workgroup.  (fine cut.)
    static constexpr int kFineCutMinBlocksPerWorkgroup = 48;
    int fine_cut = 1;                      // as coarse_cut, for the depth-ordered full f32 launch of a plain image render whose sigma and rgb go to the compositor alone (MlpArgs.fine_cut); NERF_FINE_CUT=0 / 2 at nerf_create (or NERF_DEBUG_ZSKIP=1: off)
    bool debug_fine_cut = false;           // NERF_DEBUG_FINE_CUT=1 at nerf_create: every fine-cut launch counts the tiles it did not evaluate in BUF_CUT and prints them (synchronises: a diagnostic)
    size_t max_rays_per_pass = (size_t)1 << 20;
    std::vector<hipEvent_t> ev_pool;
    std::vector<nerfint::EvPair> last_render; // events of the last render
    std::vector<nerfint::EvPair> dominant;    // accumulated dominant-kernel events (nerf_kernel_time_query)
};

namespace nerfint {

// records the message on the context (if any) and for nerf_last_error(NULL) of this thread; returns `code`
int fail(nerf_ctx *c, int code, const std::string &msg);

#define HIP_TRY(c, expr)                                                                                    \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess)                                                                               \
            return fail((c), NERF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));              \
    } while (0)

struct DeviceGuard { // a context is bound to one device; entry points may be called with another one current
    int prev = -1;
    bool ok;
    explicit DeviceGuard(int dev) {
        ok = hipGetDevice(&prev) == hipSuccess;
        if (ok && prev != dev) ok = hipSetDevice(dev) == hipSuccess; else if (ok) prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// Rows of band i of n of a window of h rows (nerf_render_opts.band_*): stripe == 0 contiguous bands, stripe > 0 stripes round-robin.
inline int band_rows(int h, int i, int n, int stripe) {
    if (n <= 1) return h;
    if (stripe <= 0) return h / n + (i < h % n ? 1 : 0);
    const int full = h / stripe, tail = h % stripe;
    return (full / n + (i < full % n ? 1 : 0)) * stripe + (tail > 0 && full % n == i ? tail : 0);
}
inline int band_first_row(int h, int i, int n) { return i * (h / n) + std::min(i, h % n); } // contiguous bands only

inline void copy3(float *dst, const float *src) { dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; } // an origin, a colour

// No C++ exception may cross the C ABI (a Rust caller would abort): every entry point that can allocate is a function-try-block.
#define NERF_CATCH(c)                                                                                              \
    catch (const std::bad_alloc &) { return fail((c), NERF_ERR_IO, "out of host memory"); }                         \
    catch (const std::exception &e) { return fail((c), NERF_ERR_INVALID, std::string("internal error: ") + e.what()); } \
    catch (...) { return fail((c), NERF_ERR_INVALID, "internal error"); }

// ---- nerf_context.cpp -------------------------------------------------------------------------------------------------------------
// the pass workspace (BUF_DIRS .. BUF_RGBF) for `rays` rays of nc coarse and m fine-pass samples; BUF_RGBC only when need_rgbc
int ensure_workspace(nerf_ctx *c, size_t rays, size_t nc, size_t m, bool need_rgbc);
// A StageLayout over one buffer of the context and a stream: what a host-pointer entry point does around its launches.
struct Staging : StageLayout {
    nerf_ctx *c; DevBuf &buf; hipStream_t st;
    Staging(nerf_ctx *c_, BufId id, hipStream_t st_) : c(c_), buf(c_->buf[id]), st(st_) {}
    template <class T = float>
    T *at(int part) const { return StageLayout::at<T>(buf.p, part); }
    int begin();  // grows the buffer to the layout's total, then issues the uploads and the fills
    int finish(); // issues the downloads, then the one hipStreamSynchronize
};
hipEvent_t get_event(nerf_ctx *c);
// returns last_render's own pairs to the pool (EvPair::dominant) and forgets the rest
void recycle_render(nerf_ctx *c);
void recycle_dominant(nerf_ctx *c, size_t keep);

// Record kernel(s) between two events of the given kind.  If done() is never reached (a launch failed and the caller
// returned early) the destructor hands the events back to the pool.
struct Timed {
    nerf_ctx *c; hipStream_t st; EvPair p; bool on = true;
    Timed(nerf_ctx *c_, hipStream_t st_, EvKind kind, uint64_t points) : c(c_), st(st_) {
        p.kind = kind; p.dominant = false; p.points = points; p.a = get_event(c); p.b = get_event(c);
        if (!p.a || !p.b) on = false;
        if (on) (void)hipEventRecord(p.a, st);
    }
    Timed(const Timed &) = delete;
    Timed &operator=(const Timed &) = delete;
    void done(std::vector<EvPair> &dst) {
        if (on) { (void)hipEventRecord(p.b, st); dst.push_back(p); p.a = p.b = nullptr; }
    }
    ~Timed() {
        if (p.a) c->ev_pool.push_back(p.a);
        if (p.b) c->ev_pool.push_back(p.b);
    }
};
// fn (-> int, a status) between two events of `kind` in c->last_render
template <class F>
int timed(nerf_ctx *c, hipStream_t st, EvKind kind, uint64_t points, F &&fn) {
    Timed t(c, st, kind, points);
    const int rc = fn();
    if (rc) return rc;
    t.done(c->last_render);
    return NERF_OK;
}

// ---- nerf_networks.cpp: one record per arithmetic -- which stream it reads and which kernels run it ---------------------------------------
inline bool valid_dtype(int d) { return d == NERF_MLP_F32 || d == NERF_MLP_BF16 || d == NERF_MLP_BF16X3 || d == NERF_MLP_F16X2; }
inline bool split_dtype(int d) { return d == NERF_MLP_BF16X3 || d == NERF_MLP_F16X2; } // f32-accurate operand-splitting arithmetics
struct Arith {
    NetBuf stream, small;    // the f32 kernels read the folded image and its small block, every other arithmetic the packed image's
    hipError_t (*init[2])(); // the dynamic-LDS attributes of the fused and of the ray-sequential kernels
    hipError_t (*fused)(const MlpArgs &, bool full, int n_blocks, hipStream_t);
    hipError_t (*trunk)(const SeqArgs &, bool export_live, int n_blocks, hipStream_t); // skip_dead: ray-sequential trunk ...
    hipError_t (*colour)(const ColourArgs &, int n_blocks, hipStream_t);               // ... and the colour head of its second launch; NULL: in the trunk launch
    size_t h8_sample_bytes;            // what the trunk exports per live sample for the colour launch: 0, 512 (packed bf16) or 1024 (f32 tiles)
    size_t (*h8_bytes)(size_t samples); // ... and the export buffer for so many samples
    bool counts_range;                 // its launches count the points that left its range (BUF_NONFINITE)
};
const Arith &arith_of(int dtype); // dtype: valid_dtype
inline bool available(const DevNet &n, int dtype) { return n.buf[arith_of(dtype).stream].p != nullptr; } // of a loaded network: all but NERF_MLP_F16X2 always are
// certify_zero's 16-bit pre-filter (cert_pass, nerf_stage_prefilter*): bf16, or f16 where the network fits its range; sigma-only launches
// on the packed image's small block.  The f16 twin counts the wave tiles in which an activation left the f16 range.
struct Prefilter {
    NetBuf stream;
    hipError_t (*init)(); // NULL: the arithmetic's own
    hipError_t (*fused)(const MlpArgs &, bool full, int n_blocks, hipStream_t);
    hipError_t (*trunk)(const SeqArgs &, bool export_live, int n_blocks, hipStream_t);
    bool counts_range;
};
const Prefilter &prefilter_of(bool f16);
// What a launch of network n in arithmetic dtype takes from the network and the context: stream, small block, zero-step skipping (f32 kernels;
// per network, decided at load), the range counter and, for MlpArgs, the context's four launch switches (ray grouping, wave tiling, depth order,
// tile rotation: the ray-mode launcher of the f32 kernels reads them; tiling also needs rays_per_row, which only an image pass knows)
void fill_net(const nerf_ctx *c, const DevNet &n, int dtype, MlpArgs &a);
void fill_net(const nerf_ctx *c, const DevNet &n, int dtype, SeqArgs &a);
hipError_t init_mlp_kernels(); // every record's init, on the current device
inline hipError_t launch_mlp(const nerf_ctx *c, int dtype, const MlpArgs &a, bool full, hipStream_t st) { return arith_of(dtype).fused(a, full, c->n_cus, st); }
// largest batch of nerf_forward_batch*: INT32_MAX minus (persistent workgroups + 1) tiles of the widest kernel (256 points)
inline size_t max_batch_points(int n_cus) { return (size_t)0x7fffffff - ((size_t)n_cus + 1) * 256; }
// the f32 sigma-only MLP_MODE_POINTS launch (nerf_density_batch's) over n points
hipError_t launch_sigma_points(const nerf_ctx *c, const DevNet &net, const float *d_pts, size_t n, float *d_sigma, hipStream_t st);

// ---- nerf_render.cpp ------------------------------------------------------------------------------------------------------------------
RayGenArgs make_raygen(const nerf_camera &cam, int s);
int check_camera(nerf_ctx *c, const nerf_camera *cam);
// what the three alpha modes ask of the compositing kernel: the background it adds (NULL: the reference's white) and whether the pack
// kernel needs the opacity plane
int check_rgba8(nerf_ctx *c, const float *background, int alpha_mode, const void *out, const float **bg_composite);
// render_image on the context's device, asynchronous on `st` (synchronises only when stats != NULL); d_depth / d_opacity
// (h x w floats each, like d_out's pixels) may be NULL (nerf_render_image_aux)
// background: NULL = the reference's white (the float entry points); else 3 floats B, the colour is sum_i w_i c_i + B * (1 - opacity)
int render_device(nerf_ctx *c, const nerf_camera *cam, const nerf_render_opts *o, float *d_out, float *d_depth, float *d_opacity,
                  hipStream_t st, nerf_stats *stats, const float *background = nullptr);
// nerf_render_image_rgba8_device: render_device into the context's f32 workspace, then the pack kernel into d_rgba (h x w words);
// validates background / alpha_mode / d_rgba.  Asynchronous on `st` unless stats != NULL or certify_zero.
int render_rgba8_device(nerf_ctx *c, const nerf_camera *cam, const nerf_render_opts *o, const float *background, int alpha_mode,
                        uint8_t *d_rgba, hipStream_t st, nerf_stats *stats);
// width and rows of what a render with these options writes (the window, or one band of it); fails like the render would
int output_window(nerf_ctx *c, const nerf_camera *cam, const nerf_render_opts *o, size_t *w, size_t *h);

} // namespace nerfint

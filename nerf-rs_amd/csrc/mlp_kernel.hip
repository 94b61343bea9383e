// mlp_kernel.hip -- fused NeRF MLP forward for gfx950 (MI355X), fp32 MFMA.
//
// Replaces Network::forward_batch (reference src/network.rs:197-237) and, in ray mode, the point fill of
// render_block (src/lib.rs:392-402, 432-443): p = origin + d_hat * t.
//
// Structure (see mlp_layout.h for the data layout):
//   * one persistent 256-thread workgroup per CU, 4 waves, each wave owns 32 points per tile;
//   * a wave's activations (256 features x 32 points) live in 128 registers in the C/D layout of
//     v_mfma_f32_32x32x2_f32; that layout IS the B-operand layout of the next layer's MFMA once the
//     weight rows are permuted (done once on the host), so activations never touch LDS or HBM;
//   * ReLU is applied on the consumer side (one v_max per k-step, hidden under 8 MFMAs);
//   * biases initialise the accumulators (as the reference does: fill_with_bias, src/network.rs:149-159);
//   * the packed weight stream (2.3 MB, L2-resident) is DMA'd global->LDS (global_load_lds_dwordx4)
//     in 16-KiB chunks into a 3-slot ring shared by the 4 waves; one s_barrier per chunk, placed in the
//     middle of the chunk so the next chunk's first operands can be fetched before they are needed;
//   * alpha (N=1) and rgb (N=3) heads run on the VALU from the register-resident activations.
//   * the bottleneck layer (no activation, src/network.rs:218) is folded into the viewdirs layer on the host, once per loaded
//     network (host_util.cpp fold_network): the colour head is relu(h7) -> viewdirs' -> rgb.
//   * k-steps of the 256-wide layers whose ReLU'd B register is zero on all 64 lanes are skipped, exactly (mlp_f32_core.hip.h
//     tile_steps; MlpArgs.zero_skip).
//   * in ray mode the four waves of a workgroup take the same 32-sample segment of four neighbouring rays (mlp_layout.h ray grouping):
//     they meet at every chunk's barrier, and rays of like depth have like numbers of dead k-steps.
//   * in the ray-mode launches of an image pass a wave's 32 points are a few consecutive samples of each ray of a small block of pixels
//     (mlp_layout.h wave tiling), not 32 samples of one ray: points that lie close together share dead hidden units, so more k-steps are
//     zero on all of the wave's columns.  Only the slot a lane loads from and stores to changes; nothing enters the MFMA stream.
//   * in the full ray-mode launch of an image pass the waves are cut from the depth-sorted samples of 8 x 4 pixel blocks instead (mlp_layout.h
//     depth ordering; the pass's order table comes from sampling_kernels.hip k_depth_order): a ray places its fine samples where its own
//     densities are, so depth, not the sample index, says which samples of neighbouring rays lie together.
//   * the persistent workgroups rotate through the tiles of a round (mlp_layout.h rotated_tile), so that tiles whose cost follows their
//     position in the launch (sample index, depth rank) are spread over all workgroups.
//   * the sigma-only ray-mode launch whose densities only the resampler reads walks the samples of each 8 x 4 pixel block front to back and
//     leaves the block once all its 32 rays are behind the reference's T < 1e-4 cut (mlp_layout.h coarse cut; the CUT instantiation): the
//     resampler gives those samples the weight 0 whatever their density.
//   * the depth-ordered full launch whose outputs only the compositor reads walks each block's ordered tiles front to back likewise and leaves
//     the block once all its rays are cut (mlp_layout.h fine cut; the FULL CUT instantiation): k_composite gives those samples the weight 0.
// Per 32-point wave tile: at most 8256 MFMAs (full; 9280 before the fold) / 7680 (sigma only) x 64 cycles.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "mlp_f32_core.hip.h"
#include "mlp_kernel.h"
#include "sample_alpha.hip.h"

using namespace nerfmlp;
using namespace mlpdev;

using namespace mlpf32;

template <bool FULL, int MODE, bool CUT = false>
__global__ __launch_bounds__(256, 1) void nerf_mlp_kernel(const MlpArgs A) {
    static_assert(!CUT || MODE == MLP_MODE_RAYS, "the cuts belong to the ray-mode launches: sigma-only the coarse cut, full the fine cut");
    constexpr bool CCUT = CUT && !FULL, FCUT = CUT && FULL;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const LDS_AS char *lds = (const LDS_AS char *)smem;
    const LDS_AS float *small = (const LDS_AS float *)(lds + kRingSlots * kChunkBytes);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p = lane & 31;
    const int h = lane >> 5;
    const int lane16 = lane * 16;

    // resident small parameters -> LDS
    {
        float *dst = (float *)(smem + kRingSlots * kChunkBytes);
        for (int i = tid; i < kSmallFloats; i += 256) dst[i] = A.small_params[i];
    }

    Pipe P;
    P.lane16 = lane16;
    P.ring_lane = lds + lane16;
    P.ring_addr = (uint32_t)(uintptr_t)lds + wave * 4096;
    P.wr_slot_off = 0;
    P.next_off = 0;
    P.stream_bytes = (FULL ? kChunksFullFolded : kChunksSigma) * kChunkBytes;
    P.gbase = (const char *)A.wstream + wave * 4096;
    pipe_zskip_init(P, A.zero_skip);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kRingSlots - 1; ++c) pipe_issue(P);
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    unsigned long long clk0 = 0, rt0 = 0;
    if (A.clock_out) { clk0 = __builtin_amdgcn_s_memtime(); rt0 = __builtin_amdgcn_s_memrealtime(); }
    P.rd_slot_off = 0;
    P.rd_base = P.ring_lane;
#pragma unroll
    for (int j = 0; j < kLdsGroup; ++j) { // prime: operands of the first group of macro-steps (pipe_prime, written out: calling it here moves the scalar compares around the tile loop)
        P.nx[2 * j] = *(const LDS_AS f32x4 *)(P.rd_base + j * 2048);
        P.nx[2 * j + 1] = *(const LDS_AS f32x4 *)(P.rd_base + j * 2048 + 1024);
    }

    const int n_points = MODE == MLP_MODE_LIST ? list_length(A) : A.n_points; // list mode: the length lives on the device
    const int n_tiles = (n_points + kPointsPerBlock - 1) / kPointsPerBlock;
    // what load_raw fetches: the sigma-only point instance (nerf_density_batch) has no directions to read
    constexpr int LOAD = (!FULL && MODE == MLP_MODE_POINTS) ? 4 : MODE;
    // slot of this lane's point in workgroup tile T.  Ray mode: through the launch's map (mlp_layout.h ray_launch_slot: wave tiling -- a wave
    // holds a few samples of each ray of a block of pixels -- and ray grouping -- the four waves take the same stretch of four neighbouring
    // bundles / rays; MlpArgs.ray_map, all off: 128 consecutive slots); every other mode 128 consecutive slots per workgroup.  The wave-uniform
    // part (base_of) is scalar work once per tile: formed for the look-ahead, then carried over in a scalar register; the lane's part of a tiled
    // slot is formed once per kernel, and a tile costs the lanes one select and one add.
    //
    // Depth ordering (the full ray-mode launch of an image pass, mlp_layout.h DepthOrder): the first A.order_tiles workgroup tiles take their
    // slots from the pass's order table, lane p of wave w of tile T entry 128 T + 32 w + p; the launch's map describes the rows behind them,
    // shifted by A.order_points slots.  The entry is loaded TWO tiles ahead, so that the t / direction loads that depend on it can still go
    // out one tile ahead.  In this instantiation every tile's prologue pays one select more (table entry, or base + lane part as before); the
    // scalar base of the map is formed for ordered tiles too and left unused there.
    //
    // Tile rotation (mlp_layout.h rotated_tile, walked by tile_walk_next): round k's tile of this workgroup is k G + ((blockIdx.x + k) mod G);
    // scalar work once per tile.
    constexpr bool ORDER = FULL && MODE == MLP_MODE_RAYS;
    const int order_tiles = ORDER ? A.order_tiles : 0, order_points = ORDER ? A.order_points : 0;
    const int lane_part = (MODE == MLP_MODE_RAYS && A.ray_map.wt.ss) ? wave_tile_lane_part(A.ray_map.wt, p) : p;
    auto ordered = [&](int T) { return ORDER && T < order_tiles; };
    auto map_tile = [&](int T) { return ORDER ? max(T - order_tiles, 0) : T; }; // the tile's number in the launch's map
    auto base_of = [&](int T) {
        return MODE == MLP_MODE_RAYS ? order_points + ray_launch_base(A.ray_map, map_tile(T), wave) : T * kPointsPerBlock + wave * kPointsPerWave;
    };
    auto lane_of = [&](int T) { return (MODE == MLP_MODE_RAYS && ray_launch_tiled(A.ray_map, map_tile(T))) ? lane_part : p; };
    // the table entry of this lane in tile T; nothing is loaded for a tile outside the ordered region (tiles at or beyond n_tiles included).
    // Bounded like every other slot is before it becomes an address: no content of the table can make a lane read or write outside the launch.
    auto entry_of = [&](int T) {
        return ordered(T) ? (int)min(A.order_table[(size_t)T * kPointsPerBlock + wave * kPointsPerWave + p], (unsigned)order_points - 1u) : 0;
    };
    // Coarse cut (mlp_layout.h RayCutWalk; the CUT instantiation, launched for A.ray_cut alone -- every other launch of the sigma-only ray-mode
    // kernel runs the instantiation without it, whose code is what it was): the workgroup takes units -- pixel blocks of
    // block_tiles consecutive tiles, then the single tiles of the untiled rows -- and walks a block's tiles front to back.  `unit` is the one under
    // way, unit_next the one held ahead (its first tile is the look-ahead of a block's last tile), unit_next2 the one the counter handed out
    // during the first tile of `unit`: thread 0 asks for it in that tile's prologue and passes it on through LDS at the tile's exchange barrier.
    // cT / cdone: the transmittance of this lane's ray behind the block's samples so far and whether it is cut (sample_alpha.hip.h), the same in
    // all four waves: each applies the tile's four alphas, which the waves exchange through LDS, in index order.  t_end: the t behind this lane's
    // sample (the next sample's, far behind the last), loaded one tile ahead with the tile's other inputs.
    const int G = gridDim.x;
    RayCutWalk cw = {0, 0, 0, 0};
    int unit = (int)blockIdx.x, unit_next = G + (int)blockIdx.x, unit_next2 = 0;
    bool unit_first = true, cdone = false;
    float cT = 1.0f, t_end_next = 0.f;
    unsigned unit_asked = 0;
    LDS_AS float *xch = (LDS_AS float *)(smem + kLdsBytes); // kCutLdsBytes behind the kernel's own, in a cut launch only
    if constexpr (CCUT) cw = ray_cut_walk_of(A.ray_map, n_points);
    // t behind the lane's sample in tile T_ of unit u_ (slot_: the lane's slot there); tiles outside the blocks have no cut
    auto t_end_of = [&](int T_, int u_, int slot_) -> float {
        if (T_ >= cw.rest_first) return 0.f;
        const int s = (T_ - u_ * cw.block_tiles) * kWavesPerBlock + wave;
        return s + 1 < A.samples_per_ray ? A.t[slot_ + 1] : A.ray_cut_far;
    };
    // Fine cut (mlp_layout.h fine_cut_walk_of; the FULL CUT instantiation, launched for A.fine_cut alone -- every other full ray-mode launch runs
    // the instantiation without it, whose code is what it was): the same units, a block being the spr / 4 ORDERED tiles of its part of the table.
    // A lane changes its ray from tile to tile here, so the walk is by ray, not by lane: the lanes that hold a point post its alpha to LDS at
    // (ray in block, sample index mod 128) and count it there; behind the tile's one barrier (the empty-tile vote's, which it replaces) lane r
    // of EVERY wave walks ray r's samples of the tile in index order -- fcur: the next index, cT / cdone as above, the same in all four waves.
    // That order is k_composite's, and a ray's samples of one tile are consecutive indices, if the ray's samples stand in the table in index
    // order: unit_flag, the block's word of A.order_flags; a block without it posts nothing and is walked to its end.  fkey: (ray in block) << 16
    // | sample index of this lane's point, formed one tile ahead with t_end.  The alphas and counts of tile k are read behind its barrier and
    // written again in front of tile k + 1's: the weight chunks' barriers of a whole trunk lie between (as for the vote's four words); the counts
    // come in two sets taken in turn, and wave 0 clears the other set behind the barrier.
    unsigned fkey_next = 0, fcur = 0;
    bool unit_flag = false, fpar = false;
    LDS_AS float *fstage = (LDS_AS float *)(smem + kLdsBytes); // kFineCutLdsBytes behind the kernel's own, in a fine-cut launch only
    if constexpr (FCUT) {
        cw = fine_cut_walk_of(order_tiles, A.samples_per_ray, n_points);
        if (tid < 64) ((unsigned *)(smem + kLdsBytes))[kFineCutCountOff + tid] = 0u; // both sets; the first tile's trunk lies in front of the first count
        unit_flag = unit < cw.blocks && A.order_flags[unit] != 0u;
    }
    // (the bodies of the fine cut's lambdas exist in its instantiation alone: in every other one they capture nothing)
    auto unit_succ = [&](int T_, int u_, int u_after) -> int { // the tile behind T_ of unit u_ when no block is cut: u_'s next one, or the first of u_after
        if constexpr (FCUT) {
            const int in_unit = ray_cut_next_in_unit(cw, u_, T_, false);
            return in_unit >= 0 ? in_unit : ray_cut_unit_tile(cw, u_after, n_tiles);
        } else return 0;
    };
    auto fine_ahead = [&](int T_, int slot_) { // fkey_next / t_end_next of the lane's point in tile T_ (slot_: its slot; an ordered tile's is below order_points)
        if constexpr (FCUT) {
            fkey_next = 0; t_end_next = 0.f;
            if (ordered(T_)) {
                const unsigned spr = (unsigned)A.samples_per_ray, rw = (unsigned)A.rays_per_row;
                const unsigned ray = (unsigned)slot_ / spr, s = (unsigned)slot_ - ray * spr, row = ray / rw, col = ray - row * rw;
                fkey_next = ((row % kDepthBlockH) * kDepthBlockW + col % kDepthBlockW) << 16 | s;
                t_end_next = s + 1u < spr ? A.t[slot_ + 1] : A.ray_cut_far;
            }
        }
    };
    const int tile0 = CUT ? ray_cut_unit_tile(cw, unit, n_tiles) : (int)blockIdx.x; // round 0's tile
    TileWalk walk = {0, 0};
    auto next_round_tile = [&]() { return tile_walk_next(walk, (int)blockIdx.x, G, A.tile_rotation != 0); };
    int tile_next = next_round_tile();  // round 1's tile (round 0's is blockIdx.x)
    int tile_next2 = next_round_tile(); // round 2's
    if constexpr (FCUT) { tile_next = unit_succ(tile0, unit, unit_next); tile_next2 = n_tiles; } // the loop forms both anew
    int base_next = base_of(tile0); // wave-uniform
    int ord_cur = entry_of(tile0), ord_next = entry_of(tile_next); // ORDER only: this lane's table entry of the coming tile and of the one behind it
    RawIn nxt = load_raw_at<LOAD>(A, ordered(tile0) ? ord_cur : base_next + lane_of(tile0)); // the next tile's t / direction are loaded one tile ahead
    if constexpr (CCUT) t_end_next = t_end_of(tile0, unit, base_next + lane_of(tile0));
    if constexpr (FCUT) fine_ahead(tile0, ordered(tile0) ? ord_cur : base_next + lane_of(tile0));
    for (int tile = tile0; tile < n_tiles; tile = tile_next, tile_next = tile_next2, tile_next2 = next_round_tile()) {
        if constexpr (FCUT) { // as below, two tiles deep: the table entry is loaded two tiles ahead
            const bool stay = ray_cut_next_in_unit(cw, unit, tile, false) >= 0;
            tile_next = unit_succ(tile, unit, unit_next);
            // the unit behind tile_next's: in a unit's first tile the counter's answer is still under way -- it is wanted there only if `unit` is
            // one tile long, a tile behind the blocks; units ascend, so every later one is such a tile too and has no table entry: "no tile" will do
            tile_next2 = unit_succ(tile_next, stay ? unit : unit_next, stay ? unit_next : unit_first ? ray_cut_units(cw) : unit_next2);
            if (unit_first && tid == 0) unit_asked = atomicAdd(A.cut_counters, 1u);
        }
        if constexpr (CCUT) { // the tile to look ahead to: the unit's next one, or the first of the unit held ahead; the unit behind that is asked for
            const int in_unit = ray_cut_next_in_unit(cw, unit, tile, false);
            tile_next = in_unit >= 0 ? in_unit : ray_cut_unit_tile(cw, unit_next, n_tiles);
            if (unit_first && tid == 0) unit_asked = atomicAdd(A.cut_counters, 1u);
        }
        const int slot = ordered(tile) ? ord_cur : base_next + lane_of(tile);
        const bool valid = slot < n_points;
        base_next = base_of(tile_next);
        if (ORDER) { ord_cur = ord_next; ord_next = entry_of(tile_next2); }
        const RawIn in = nxt;
        nxt = load_raw_at<LOAD>(A, ordered(tile_next) ? ord_cur : base_next + lane_of(tile_next)); // consumed one tile (~250 us) later
        const float t_end = t_end_next;
        const unsigned fkey = fkey_next;
        if constexpr (FCUT) fine_ahead(tile_next, ordered(tile_next) ? ord_cur : base_next + lane_of(tile_next));
        if constexpr (CCUT)
            t_end_next = t_end_of(tile_next, ray_cut_next_in_unit(cw, unit, tile, false) >= 0 ? unit : unit_next, base_next + lane_of(tile_next));
        float px, py, pz;
        point_of<MODE>(A, in, px, py, pz);
        const float dx = in.dx, dy = in.dy, dz = in.dz;
        const unsigned entry = __builtin_bit_cast(unsigned, in.b);
        const size_t i = MODE == MLP_MODE_LIST ? (size_t)(entry & 0x7fffffffu) : (size_t)slot; // where the outputs go
        // an audited certificate (certify_zero): the raw pre-activation leaves the kernel -- k_cert_audit compares it with 0
        const bool audit = MODE == MLP_MODE_LIST && (entry >> 31) != 0;

        f32x16 E[2];
        encode_point(px, py, pz, h, E);

        f32x16 X[8], Y[8];

        // dense0: 64 slots -> 256, output X
        load_bias<8>(X, small + kBiasOff + 0 * 256, h);
        tile_steps<8, false>(E[0], X, P);
        tile_steps<8, false>(E[1], X, P);

        float sigma = 0.f;
        // dense1..4
        hidden_layer<true>(X, Y, small + kBiasOff + 1 * 256, P, h);
        hidden_layer<true>(Y, X, small + kBiasOff + 2 * 256, P, h);
        hidden_layer<true>(X, Y, small + kBiasOff + 3 * 256, P, h);
        hidden_layer<true>(Y, X, small + kBiasOff + 4 * 256, P, h);
        // dense5: [encoding ; h4] -> 256 (skip connection, src/network.rs:209-210)
        load_bias<8>(Y, small + kBiasOff + 5 * 256, h);
        tile_steps<8, false>(E[0], Y, P);
        tile_steps<8, false>(E[1], Y, P);
#pragma unroll
        for (int t = 0; t < 8; ++t) tile_steps<8, true>(X[t], Y, P);
        // dense6, dense7
        hidden_layer<true>(Y, X, small + kBiasOff + 6 * 256, P, h);
        hidden_layer<true>(X, Y, small + kBiasOff + 7 * 256, P, h);
        const float pre = alpha_pre(Y, small, h);
        sigma = fmaxf(pre, 0.f);
        if (MODE == MLP_MODE_GRID) {
            if (valid && h == 0 && A.sigma_out) A.sigma_out[i] = sigma;
            if (A.occ_bits) { // fused occupancy: one word per 32-point wave tile, bit = lane (NaN > threshold is false)
                const unsigned word = (unsigned)__ballot(valid && h == 0 && sigma > A.occ_threshold);
                const int slot0 = tile * kPointsPerBlock + wave * kPointsPerWave;
                if (lane == 0 && slot0 < n_points) A.occ_bits[slot0 >> 5] = word;
            }
        } else
        if (valid && h == 0) A.sigma_out[i] = audit ? pre : sigma;
        if constexpr (CCUT) {
            // Exchange (one workgroup barrier per tile): every wave leaves its 32 alphas, thread 0 the unit it was handed; then every wave takes
            // the tile's four samples of its lanes' rays in index order, as weights_scan will.  The skip happens here, at a tile boundary, where
            // the weight stream has wrapped: the pipeline is left as it is.
            const float al = sample_alpha_of(in.a, t_end, sigma);
            LDS_AS unsigned *xch_unit = (LDS_AS unsigned *)(xch + kPointsPerBlock);
            if (h == 0) xch[wave * kPointsPerWave + p] = al;
            if (unit_first && tid == 0) *xch_unit = unit_asked;
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            if (unit_first) // the first 2 G units are the workgroups' own; clamped: a unit beyond the launch's has no tile
                unit_next2 = (int)min(2u * (unsigned)G + (unsigned)__builtin_amdgcn_readfirstlane((int)*xch_unit), (unsigned)ray_cut_units(cw));
            bool all_cut = false;
            if (tile < cw.rest_first) {
#pragma unroll
                for (int w = 0; w < kWavesPerBlock; ++w) transmittance_step(cT, cdone, xch[w * kPointsPerWave + p]);
                all_cut = __all(cdone || !valid) != 0; // a lane without a sample counts as cut
            }
            if (ray_cut_next_in_unit(cw, unit, tile, all_cut) < 0) { // on to the unit held ahead
                const int end = (unit + 1) * cw.block_tiles;
                if (all_cut && tile + 1 < end) {
                    // cut with tiles left: their samples get sigma = 0 (the buffer is defined and the same from frame to frame) -- thread (ray, j)
                    // of 32 x 8 writes every eighth sample index of its ray; the inputs loaded ahead were the next tile's: take the next unit's
                    const int s0 = (tile + 1 - unit * cw.block_tiles) * kWavesPerBlock;
                    float *row = A.sigma_out + (wave_tile_base_slot(A.ray_map.wt, unit * cw.block_tiles, 0) + wave_tile_lane_part(A.ray_map.wt, tid >> 3));
                    for (int s = s0 + (tid & 7); s < A.samples_per_ray; s += 8) row[s] = 0.f;
                    if (A.cut_count && tid == 0) atomicAdd((unsigned long long *)(A.cut_counters + 2), (unsigned long long)(end - tile - 1));
                    tile_next = ray_cut_unit_tile(cw, unit_next, n_tiles);
                    base_next = base_of(tile_next);
                    nxt = load_raw_at<LOAD>(A, base_next + lane_of(tile_next));
                    t_end_next = t_end_of(tile_next, unit_next, base_next + lane_of(tile_next));
                }
                unit = unit_next; unit_next = unit_next2; unit_first = true;
                cT = 1.0f; cdone = false;
            } else unit_first = false;
        }
        bool fine_any = true, fine_leave = false, fine_all_cut = false;
        if constexpr (FCUT) {
            // Exchange (the tile's one workgroup barrier, shared with the empty-tile vote): the alphas by (ray, sample index) and their number per
            // ray, the waves' votes, thread 0 the unit it was handed; then lane r of every wave walks ray r.  What follows from the walk -- leaving
            // the block -- happens at the END of the tile (fine_tile_end), behind the colour head or the vote's pipe_restart.
            LDS_AS unsigned *fcnt = (LDS_AS unsigned *)fstage + kFineCutCountOff + (fpar ? 32 : 0);
            LDS_AS unsigned *fcnt_other = (LDS_AS unsigned *)fstage + kFineCutCountOff + (fpar ? 0 : 32);
            LDS_AS unsigned *xch_unit = (LDS_AS unsigned *)fstage + kFineCutUnitOff;
            LDS_AS int *vote = (LDS_AS int *)(lds + kRingSlots * kChunkBytes) + kMiscOff + 8; // the empty-tile vote's four words
            const bool walked = unit_flag && tile < cw.rest_first; // wave-uniform
            if (walked && h == 0) {
                const unsigned r = fkey >> 16; // < 32
                fstage[r * kFineCutRowWords + (fkey & (kPointsPerBlock - 1))] = sample_alpha_of(in.a, t_end, sigma);
                __hip_atomic_fetch_add((unsigned *)(fcnt + r), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            const bool any_wave = __any(valid && sigma > 0.0f);
            if (lane == 0) vote[wave] = any_wave ? 1 : 0;
            if (unit_first && tid == 0) *xch_unit = unit_asked;
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            if (unit_first) // the first 2 G units are the workgroups' own; clamped: a unit beyond the launch's has no tile
                unit_next2 = (int)min(2u * (unsigned)G + (unsigned)__builtin_amdgcn_readfirstlane((int)*xch_unit), (unsigned)ray_cut_units(cw));
            fine_any = (vote[0] | vote[1] | vote[2] | vote[3]) != 0;
            const unsigned n_mine = min(fcnt[p], (unsigned)kPointsPerBlock); // ray p's samples in this tile: indices fcur .. fcur + n_mine - 1
            for (unsigned k = 0; k < n_mine; ++k)
                transmittance_step(cT, cdone, fstage[p * kFineCutRowWords + ((fcur + k) & (kPointsPerBlock - 1))]);
            fcur += n_mine;
            if (tid < 32) fcnt_other[tid] = 0u; // the next tile's set: last read behind the previous tile's barrier
            fpar = !fpar;
            fine_all_cut = walked && __all(cdone) != 0;
            fine_leave = ray_cut_next_in_unit(cw, unit, tile, fine_all_cut) < 0;
        }
        auto fine_tile_end = [&]() { // FCUT: the tile is done, its outputs are on their way; the weight stream stands at chunk 0 of the next tile
          if constexpr (FCUT) {
            if (!fine_leave) { unit_first = false; return; }
            const int end = (unit + 1) * cw.block_tiles;
            if (fine_all_cut && tile + 1 < end) {
                // cut with tiles left: the points of their table entries get sigma = 0 and rgb = 0 (k_composite multiplies them by the weight 0: the
                // buffers hold finite values, the same from frame to frame); the entries and inputs loaded ahead were the block's: take the next unit's
                for (size_t q = (size_t)(tile + 1) * kPointsPerBlock + tid; q < (size_t)end * kPointsPerBlock; q += 256) {
                    const size_t e = min(A.order_table[q], (unsigned)order_points - 1u);
                    A.sigma_out[e] = 0.f;
                    A.rgb_out[3 * e + 0] = 0.f; A.rgb_out[3 * e + 1] = 0.f; A.rgb_out[3 * e + 2] = 0.f;
                }
                if (A.cut_count && tid == 0) atomicAdd((unsigned long long *)(A.cut_counters + 2), (unsigned long long)(end - tile - 1));
                tile_next = ray_cut_unit_tile(cw, unit_next, n_tiles);
                tile_next2 = unit_succ(tile_next, unit_next, unit_next2);
                ord_cur = entry_of(tile_next); ord_next = entry_of(tile_next2);
                base_next = base_of(tile_next);
                const int slot_next = ordered(tile_next) ? ord_cur : base_next + lane_of(tile_next);
                nxt = load_raw_at<LOAD>(A, slot_next);
                fine_ahead(tile_next, slot_next);
            }
            unit = unit_next; unit_next = unit_next2; unit_first = true;
            cT = 1.0f; cdone = false; fcur = 0;
            unit_flag = unit < cw.blocks && A.order_flags[unit] != 0u;
          }
        };
        if (FULL && (A.skip_empty || A.empty_vote)) {
            // Empty-tile skip (exact): if sigma == 0 for all 128 points of this workgroup's tile, then
            // alpha = 1 - exp(-0 * delta) = 0 and w = T * 0 = 0 exactly for each of them (src/lib.rs:271-272), so their
            // colours never reach a pixel: skip viewdirs' + rgb (6.9 % of a full evaluation), write rgb = 0.
            LDS_AS int *vote = (LDS_AS int *)(lds + kRingSlots * kChunkBytes) + kMiscOff + 8;
            bool any_wg = fine_any;
            if constexpr (!FCUT) any_wg = tile_has_density(vote, valid && sigma > 0.0f, wave, lane);
            if (!any_wg) {
                if (valid && h == 0) {
                    A.rgb_out[3 * (size_t)i + 0] = 0.f; A.rgb_out[3 * (size_t)i + 1] = 0.f; A.rgb_out[3 * (size_t)i + 2] = 0.f;
                }
                if (A.skip_counter && tid == 0) atomicAdd(A.skip_counter, 1ull);
                pipe_restart(P);
#if NERF_DIAG_RESTART_TWICE // timing-only variant (make variant): a second, idle restart -- the frame-time difference prices one
                pipe_restart(P);
#endif
                if constexpr (FCUT) fine_tile_end();
                continue;
            }
        }
        if (FULL) {
            f32x16 D;
            encode_dir(dx, dy, dz, h, D);
            // viewdirs': [relu(h7) ; dir encoding] -> 128 = bottleneck (no activation, :218) folded into viewdirs (:219-222);
            // W' and b' come from the host (mlp_layout.h kChunksFullFolded)
            f32x16 V[4];
            load_bias<4>(V, small + kBiasViewOff, h);
#pragma unroll
            for (int t = 0; t < 8; ++t) tile_steps<4, true>(Y[t], V, P);
            tile_steps<4, false>(D, V, P);
            float c[3];
            rgb_head(V, small, h, c);
            if (valid && h == 0) {
                A.rgb_out[3 * (size_t)i + 0] = c[0];
                A.rgb_out[3 * (size_t)i + 1] = c[1];
                A.rgb_out[3 * (size_t)i + 2] = c[2];
            }
        }
        if constexpr (FCUT) fine_tile_end();
    }
    // drain the (unused) prefetches before the LDS allocation is released
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    pipe_zskip_report(P, A.zskip_stats, lane);
    if (A.clock_out && tid == 0) { // diagnostic: shader clock = d(memtime) / d(memrealtime) x 100 MHz
        A.clock_out[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - clk0;
        A.clock_out[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - rt0;
    }
}

// NERF_DEBUG_ZSKIP: the {executed, total} ReLU k-step counters of one launch.  Cleared in front of it, read (synchronising) and printed
// behind it -- the clear, the atomics and the synchronising read are a diagnostic, never on in timed runs (the kernels keep their
// per-wave sums in scalar registers regardless: mlp_f32_core.hip.h Pipe).
hipError_t nerf_zskip_clear(unsigned long long *stats, hipStream_t stream) {
    return stats ? hipMemsetAsync(stats, 0, 2 * sizeof(unsigned long long), stream) : hipSuccess;
}
hipError_t nerf_zskip_print(const char *what, unsigned long long *stats, hipStream_t stream) {
    if (!stats) return hipSuccess;
    unsigned long long h[2] = {0, 0};
    hipError_t e = hipMemcpyAsync(h, stats, sizeof h, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) fprintf(stderr, "nerf zskip: %s relu_ksteps_executed=%llu relu_ksteps_total=%llu\n", what, h[0], h[1]);
    return e;
}

template <bool FULL, int MODE, bool CUT = false>
static hipError_t launch_t(const MlpArgs &a, int n_blocks, hipStream_t stream, int lds_bytes = kLdsBytes) {
    hipError_t e = nerf_zskip_clear(a.zskip_stats, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((nerf_mlp_kernel<FULL, MODE, CUT>), dim3(n_blocks), dim3(256), lds_bytes, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    static const char *const modes[4] = {"points", "rays", "list", "grid"};
    char what[48];
    snprintf(what, sizeof what, "nerf_mlp_kernel<%s,%s>", FULL ? "full" : "sigma", modes[MODE]);
    return nerf_zskip_print(what, a.zskip_stats, stream);
}

hipError_t nerf_mlp_init() {
    // sigma-only in point mode is nerf_density_batch, in grid mode nerf_density_grid (no colour on a lattice)
    const void *ks[9] = {(const void *)nerf_mlp_kernel<true, MLP_MODE_POINTS>, (const void *)nerf_mlp_kernel<true, MLP_MODE_RAYS>,
                         (const void *)nerf_mlp_kernel<false, MLP_MODE_RAYS>, (const void *)nerf_mlp_kernel<true, MLP_MODE_LIST>,
                         (const void *)nerf_mlp_kernel<false, MLP_MODE_LIST>, (const void *)nerf_mlp_kernel<false, MLP_MODE_POINTS>,
                         (const void *)nerf_mlp_kernel<false, MLP_MODE_GRID>, (const void *)nerf_mlp_kernel<false, MLP_MODE_RAYS, true>,
                         (const void *)nerf_mlp_kernel<true, MLP_MODE_RAYS, true>};
    for (int i = 0; i < 9; ++i) {
        hipError_t e = hipFuncSetAttribute(ks[i], hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes + (i == 7 ? kCutLdsBytes : i == 8 ? kFineCutLdsBytes : 0)); // the cut instantiations' exchange
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// Every ray-mode launch comes through here (plain and skip_empty renders, shared-origin ray batches, coarse and fine passes): the wave
// tiling and ray grouping of this launch, from its shape and the context's switches (MlpArgs.wave_tiling, .ray_grouping).  The pixel block
// depends on the kind of launch (mlp_layout.h kWaveTileSigma* / kWaveTileFull*); a launch without rays_per_row (a ray batch) is never tiled.
// A full launch whose caller built the pass's depth-order table (MlpArgs.order_table; nerf_render.cpp eval_net) takes the first (rows / 4) * 4
// rows from it and maps the rows behind them like a launch of their own.
static hipError_t launch_mlp_rays(const MlpArgs &a, bool full, int n_blocks, hipStream_t stream) {
    MlpArgs g = a;
    // depth ordering: the first (rows / 4) * 4 rows of a qualifying full launch whose caller built the pass's table; the map covers the rest
    DepthOrder d = {0, 0, 0, 0};
    if (a.order_table) d = nerf_mlp_depth_order(a, full);
    g.order_tiles = d.tiles; g.order_points = d.points;
    if (!d.tiles) g.order_table = nullptr;
    g.ray_map = ray_launch_map_of(a.n_points - d.points, a.samples_per_ray, a.rays_per_row, full, a.ray_grouping != 0, a.wave_tiling != 0);
    // the coarse cut (mlp_layout.h RayCutWalk): the tiled region ungrouped, the workgroups take units from the context's counter
    g.ray_cut = 0;
    if (a.ray_cut) {
        const RayCutWalk w = nerf_mlp_ray_cut(a, full);
        if (w.blocks > 0) {
            g.ray_cut = 1;
            g.ray_map = ray_cut_map_of(g.ray_map);
            if (n_blocks > ray_cut_units(w)) n_blocks = ray_cut_units(w);
            const hipError_t e = hipMemsetAsync(a.cut_counters, 0, sizeof(unsigned int), stream);
            if (e != hipSuccess) return e;
            return launch_t<false, MLP_MODE_RAYS, true>(g, n_blocks, stream, kLdsBytes + kCutLdsBytes);
        }
    }
    // the fine cut (mlp_layout.h fine_cut_walk_of): the ordered launch as it is mapped above, its workgroups take units from the same counter
    g.fine_cut = 0;
    if (a.fine_cut && d.tiles) {
        const RayCutWalk w = nerf_mlp_fine_cut(a, full);
        if (w.blocks > 0) {
            g.fine_cut = 1;
            if (n_blocks > ray_cut_units(w)) n_blocks = ray_cut_units(w);
            const hipError_t e = hipMemsetAsync(a.cut_counters, 0, sizeof(unsigned int), stream);
            if (e != hipSuccess) return e;
            return launch_t<true, MLP_MODE_RAYS, true>(g, n_blocks, stream, kLdsBytes + kFineCutLdsBytes);
        }
    }
    return full ? launch_t<true, MLP_MODE_RAYS>(g, n_blocks, stream) : launch_t<false, MLP_MODE_RAYS>(g, n_blocks, stream);
}

hipError_t nerf_mlp_launch(const MlpArgs &a, bool full, int n_blocks, hipStream_t stream) {
    if (a.n_points <= 0) return hipSuccess;
    const int n_tiles = (a.n_points + kPointsPerBlock - 1) / kPointsPerBlock;
    if (n_blocks > n_tiles) n_blocks = n_tiles;
    if (n_blocks < 1) n_blocks = 1;
    if (a.mode == MLP_MODE_LIST) {
        if (!a.point_list || !a.point_list_count) return hipErrorInvalidValue;
        return full ? launch_t<true, MLP_MODE_LIST>(a, n_blocks, stream) : launch_t<false, MLP_MODE_LIST>(a, n_blocks, stream);
    }
    if (a.mode == MLP_MODE_GRID) {
        if (full || a.grid_n[0] <= 0 || a.grid_n[1] <= 0 || a.grid_n[2] <= 0 || (!a.sigma_out && !a.occ_bits)) return hipErrorInvalidValue;
        const unsigned long long plane = (unsigned long long)a.grid_n[0] * (unsigned long long)a.grid_n[1];
        if (plane > (unsigned long long)a.n_points || plane * (unsigned long long)a.grid_n[2] != (unsigned long long)a.n_points) return hipErrorInvalidValue;
        return launch_t<false, MLP_MODE_GRID>(a, n_blocks, stream);
    }
    if (a.mode == MLP_MODE_POINTS)
        return full ? launch_t<true, MLP_MODE_POINTS>(a, n_blocks, stream) : launch_t<false, MLP_MODE_POINTS>(a, n_blocks, stream);
    return launch_mlp_rays(a, full, n_blocks, stream);
}

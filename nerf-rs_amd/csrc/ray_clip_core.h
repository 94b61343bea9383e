// ray_clip_core.h -- one ray against an occupancy grid: the slab test and the cell walk of nerf_clip_rays, written once for the device
// (ray_clip_kernels.hip: one lane per ray) and for the host (nerf_debug_clip_rays in nerf_host_api.cpp).  The contract -- every rounding --
// is in include/nerf_mi355x.h, "ray clipping"; tests/helpers/ray_clip.py restates it.  No HIP header is needed: under hipcc the functions
// are __host__ __device__, elsewhere plain inline C++.  Every translation unit that includes this is built with -ffp-contract=off, so that
// each operation below is one f32 operation rounded once on either side; division and sqrtf are correctly rounded on both.
// Scalars and selects instead of arrays indexed by the walk's axis: nothing here needs scratch memory on the device.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NERF_CLIP_HD __host__ __device__ inline
#else
#define NERF_CLIP_HD inline
#endif

namespace nerfclip {

// max and min as the contract defines them: a NaN in `a` is dropped, one in `b` is kept -- the same on every side, unlike fmaxf
NERF_CLIP_HD float maxf(float a, float b) { return a > b ? a : b; }
NERF_CLIP_HD float minf(float a, float b) { return a < b ? a : b; }

// what nerf_clip_rays* and nerf_render_rays_clipped* refuse about the grid, in the header's order: the message, or NULL if it passes
inline const char *check_grid(const void *occ_bits, const float *lo, const float *step, const int32_t *dims) {
    if (!occ_bits || !lo || !step || !dims) return "occ_bits, lo, step and dims must not be NULL";
    for (int k = 0; k < 3; ++k)
        if (dims[k] < 1) return "dims must be positive";
    for (int k = 0; k < 3; ++k)
        if (!(lo[k] - lo[k] == 0.0f)) return "lo must be finite";
    for (int k = 0; k < 3; ++k)
        if (!(step[k] - step[k] == 0.0f) || !(step[k] > 0.0f)) return "step must be finite and greater than 0";
    const unsigned long long plane = (unsigned long long)dims[0] * (unsigned long long)dims[1];
    if (plane > 0x7fffffffull || plane * (unsigned long long)dims[2] > 0x7fffffffull) return "grid too large: dims[0] * dims[1] * dims[2] must be at most INT32_MAX";
    return nullptr;
}

// what nerf_clip_rays* refuses about the rays, after the grid
inline const char *check_rays(const void *origins, size_t n_origins, const void *dirs, size_t n_rays, float near_, float far_, const void *bounds,
                              const void *bounds_out, const void *hit_out) {
    if (n_rays > (size_t)0x7fffffff) return "n_rays must be at most INT32_MAX";
    if (n_rays > 0 && (!origins || !dirs || !bounds_out || !hit_out)) return "origins, dirs, bounds_out and hit_out must not be NULL";
    if (n_origins != 1 && n_origins != n_rays) return "n_origins must be 1 (one origin for every ray) or n_rays";
    if (!bounds) {
        if (!(near_ - near_ == 0.0f) || !(far_ - far_ == 0.0f)) return "near_ and far_ must be finite when bounds is NULL";
        if (!(far_ > near_)) return "far_ must be greater than near_ when bounds is NULL";
    }
    return nullptr;
}

// the direction the walk (and the networks) see: dirs[r], or Vec3::normalize as k_batch_prepare applies it
NERF_CLIP_HD void direction(const float *v, int normalize, float *d) {
    if (normalize) {
        const float len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        d[0] = v[0] / len; d[1] = v[1] / len; d[2] = v[2] / len;
    } else {
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2];
    }
}

// plane k of an axis: P(k) = fl(G_lo + fl(step * (float)k))
NERF_CLIP_HD float plane(float g_lo, float step, int k) { return g_lo + step * (float)k; }
// the next crossing of an axis, always from the plane's index: fl(fl(P(i + (s > 0)) - o) * inv); +inf for an axis the ray does not move along
NERF_CLIP_HD float crossing(float g_lo, float step, int i, int s, float o, float inv) {
    return s == 0 ? INFINITY : (plane(g_lo, step, i + (s > 0 ? 1 : 0)) - o) * inv;
}
// i = clamp(floor(q), 0, n - 1), a NaN to 0
NERF_CLIP_HD int entry_index(float q, int n) {
    if (q != q) return 0;
    const float f = floorf(q);
    if (!(f > 0.0f)) return 0;
    if (f >= (float)(n - 1)) return n - 1;
    return (int)f;
}

// The occupancy words behind a one-word cache: consecutive x steps hit the same word.  A cell index outside the grid is never read: it
// counts as empty and, for the host diagnostic, is counted.
struct Cells {
    const uint32_t *bits;
    int nx, ny, nz;
    int cached_word;
    uint32_t cached;
    uint32_t refused;
    NERF_CLIP_HD bool occupied(int ix, int iy, int iz) {
        if ((unsigned)ix >= (unsigned)nx || (unsigned)iy >= (unsigned)ny || (unsigned)iz >= (unsigned)nz) { ++refused; return false; }
        const int cell = ix + nx * (iy + ny * iz); // < N <= INT32_MAX
        const int w = cell >> 5;
        if (w != cached_word) { cached = bits[w]; cached_word = w; }
        return (cached >> (cell & 31)) & 1u;
    }
};

struct Result {
    float t_first, t_last; // the span, when hit
    int hit;               // 0 / 1
    int rounds;            // walk rounds taken (diagnostic)
    uint32_t refused;      // cell indices outside the grid that the range check kept from being read (always 0 unless the walk is wrong)
};

// One ray: origin o, direction d (already normalised if the caller asked), its [near, far].
NERF_CLIP_HD Result clip_ray(const uint32_t *bits, const float *lo, const float *step, const int32_t *dims, const float *o, const float *d,
                             float near_, float far_) {
    Result res;
    res.t_first = near_; res.t_last = far_; res.hit = 0; res.rounds = 0; res.refused = 0;
    const int n0 = dims[0], n1 = dims[1], n2 = dims[2];
    const float st0 = step[0], st1 = step[1], st2 = step[2];
    const float gl0 = lo[0] - 0.5f * st0, gl1 = lo[1] - 0.5f * st1, gl2 = lo[2] - 0.5f * st2;
    const float gh0 = lo[0] + st0 * ((float)n0 - 0.5f), gh1 = lo[1] + st1 * ((float)n1 - 0.5f), gh2 = lo[2] + st2 * ((float)n2 - 0.5f);
    const float o0 = o[0], o1 = o[1], o2 = o[2], d0 = d[0], d1 = d[1], d2 = d[2];
    // slab test
    float t_in = near_, t_out = far_;
    float inv0 = 0.0f, inv1 = 0.0f, inv2 = 0.0f;
    if (d0 == 0.0f) { if (!(gl0 <= o0 && o0 < gh0)) return res; }
    else { inv0 = 1.0f / d0; const float ta = (gl0 - o0) * inv0, tb = (gh0 - o0) * inv0; t_in = maxf(t_in, minf(ta, tb)); t_out = minf(t_out, maxf(ta, tb)); }
    if (d1 == 0.0f) { if (!(gl1 <= o1 && o1 < gh1)) return res; }
    else { inv1 = 1.0f / d1; const float ta = (gl1 - o1) * inv1, tb = (gh1 - o1) * inv1; t_in = maxf(t_in, minf(ta, tb)); t_out = minf(t_out, maxf(ta, tb)); }
    if (d2 == 0.0f) { if (!(gl2 <= o2 && o2 < gh2)) return res; }
    else { inv2 = 1.0f / d2; const float ta = (gl2 - o2) * inv2, tb = (gh2 - o2) * inv2; t_in = maxf(t_in, minf(ta, tb)); t_out = minf(t_out, maxf(ta, tb)); }
    if (!(t_in < t_out)) return res;
    // entry cell
    int i0 = entry_index(((o0 + d0 * t_in) - gl0) / st0, n0);
    int i1 = entry_index(((o1 + d1 * t_in) - gl1) / st1, n1);
    int i2 = entry_index(((o2 + d2 * t_in) - gl2) / st2, n2);
    // a NaN direction is neither > 0 nor < 0: the ray does not move along that axis
    const int s0 = d0 > 0.0f ? 1 : d0 < 0.0f ? -1 : 0, s1 = d1 > 0.0f ? 1 : d1 < 0.0f ? -1 : 0, s2 = d2 > 0.0f ? 1 : d2 < 0.0f ? -1 : 0;
    float tn0 = crossing(gl0, st0, i0, s0, o0, inv0), tn1 = crossing(gl1, st1, i1, s1, o1, inv1), tn2 = crossing(gl2, st2, i2, s2, o2, inv2);
    Cells cells;
    cells.bits = bits; cells.nx = n0; cells.ny = n1; cells.nz = n2; cells.cached_word = -1; cells.cached = 0u; cells.refused = 0u;
    float t_cur = t_in, t_first = 0.0f, t_last = 0.0f;
    int hit = 0, round = 0;
    const int max_rounds = n0 + n1 + n2 + 3; // the walk ends here whatever the floats are
    for (; round < max_rounds; ++round) {
        int a = 0;
        float m = tn0;
        if (tn1 < m) { a = 1; m = tn1; }
        if (tn2 < m) { a = 2; m = tn2; }
        const float t_exit = minf(m, t_out);
        if (t_exit > t_cur && cells.occupied(i0, i1, i2)) {
            if (!hit) { t_first = t_cur; hit = 1; }
            t_last = t_exit;
        }
        if (t_out <= m) break;
        if (a == 0) { i0 += s0; if ((unsigned)i0 >= (unsigned)n0) break; }
        else if (a == 1) { i1 += s1; if ((unsigned)i1 >= (unsigned)n1) break; }
        else { i2 += s2; if ((unsigned)i2 >= (unsigned)n2) break; }
        t_cur = maxf(t_cur, m);
        if (a == 0) tn0 = crossing(gl0, st0, i0, s0, o0, inv0);
        else if (a == 1) tn1 = crossing(gl1, st1, i1, s1, o1, inv1);
        else tn2 = crossing(gl2, st2, i2, s2, o2, inv2);
    }
    res.rounds = round < max_rounds ? round + 1 : max_rounds;
    res.refused = cells.refused;
    if (hit) { res.t_first = t_first; res.t_last = t_last; res.hit = 1; }
    return res;
}

// ray r of a batch in nerf_render_rays' argument conventions: origins[r] or origins[0], dirs[r], bounds[r] or {near_, far_}
NERF_CLIP_HD Result clip_batch_ray(const uint32_t *bits, const float *lo, const float *step, const int32_t *dims, const float *origins,
                                   int per_ray_origins, const float *dirs, int normalize, float near_, float far_, const float *bounds, size_t r,
                                   float *near_r, float *far_r) {
    const float *o = per_ray_origins ? origins + 3 * r : origins;
    float d[3];
    direction(dirs + 3 * r, normalize, d);
    *near_r = bounds ? bounds[2 * r] : near_;
    *far_r = bounds ? bounds[2 * r + 1] : far_;
    return clip_ray(bits, lo, step, dims, o, d, *near_r, *far_r);
}

} // namespace nerfclip

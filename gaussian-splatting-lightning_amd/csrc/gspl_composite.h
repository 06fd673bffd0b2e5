// gspl_composite.h — device helpers shared by the compositing kernels (composite.hip: forward + per-splat statistics;
// composite_bwd.hip: backward; features.hip: wide features), among them the one definition of the 8x8 block walk.  gfx950, wave64.
//
// The compositing rule restated here is the published 3DGS rule with the per-API constants of SURVEY.md Appendix B (ModeTraits
// in gspl_device.h); call sites replaced: internal/renderers/gsplat_v1_renderer.py:588-601 (`rasterize_to_pixels`),
// gsplat_renderer.py:86-99 (`rasterize_gaussians`), vanilla_renderer.py:111-120 (Inria `GaussianRasterizer`).
#pragma once
#include "gspl_device.h"
#include "gspl_host.h"
#include "gspl_rowtile.h"

namespace gspl {

static constexpr int TILE = 16;

typedef float v2f __attribute__((ext_vector_type(2)));

// sigma = 0.5 (a dx^2 + c dy^2) + b dx dy, evaluated in the FACTORED form
//     sigma = ha u^2 + hd dy^2,   u = dx + k dy,   ha = a / 2,  k = b / a,  hd = (c - b^2 / a) / 2 = det / (2 a).
// Why (round 5): the three-term form cancels.  A long anisotropic splat (a trained scene's "needles": footprints of hundreds of
// pixels, a c / det ~ 1e4) has a dx^2, c dy^2 and 2 b dx dy ~ 1e5-1e6 each for a sum of ~5 on its ridge, and fp32 then carries an
// absolute error of 1e-3 ... 4e-2 in sigma — 0.1 ... 4 % in alpha, far outside the 2e-5 band in which the oracle calls a 1/255
// decision fragile (tests/test_locked_parity.py on `synthetic.scene_surfaces`: robust pixels off by one flipped splat, 2.8e-3).
// Both terms of the factored form are products of the same sign; what is left is the rounding of u (1e-7 x the distance to the
// centre): measured worst |d sigma| over the 3000 largest splats of that scene 1.5e-3 -> 1e-5.  Same instruction count per pixel
// pair.  The forward and the backward evaluate bit-identical values (their skip / stop decisions must agree): explicit fma, one
// definition, and the per-splat factors come from `sigma_coef` in both.
struct SigmaCoef { float ha, k, hd; };
// (conic_det: gspl_device.h — a c - b^2 without the cancellation of its two products)
__device__ __forceinline__ SigmaCoef sigma_coef(float a, float b, float c) {
    SigmaCoef s;
    s.ha = 0.5f * a;
    if (a != 0.f) {
        // k: a correctly rounded division — its rounding, times the distance to the centre, is what is left of sigma's error.  hd only
        // scales the (positive, <= tau) second term: the 1-ulp hardware reciprocal is plenty
        s.k = b / a;
        s.hd = (0.5f * conic_det(a, b, c)) * __builtin_amdgcn_rcpf(a);
    } else {
        // a == 0: sigma = b dx dy + c dy^2 / 2.  With b == 0 that IS the factored form (k = 0, hd = c / 2); with b != 0 the matrix is
        // indefinite (det = -b^2 < 0) — not a Gaussian: such a splat is never composited (sigma = NaN fails every `sigma >= 0`)
        s.k = 0.f;
        s.hd = (b == 0.f) ? 0.5f * c : __builtin_nanf("");
    }
    return s;
}
__device__ __forceinline__ float eval_sigma(float ha, float k, float hd, float dx, float dy) {
    const float u = fmaf(k, dy, dx);
    return fmaf(ha * u, u, (hd * dy) * dy);
}

// Two splats (or two pixels) at once with packed fp32 math; each component is bit-identical to eval_sigma.
__device__ __forceinline__ v2f eval_sigma2(v2f ha, v2f k, v2f hd, v2f dx, v2f dy) {
    const v2f u = __builtin_elementwise_fma(k, dy, dx);
    return __builtin_elementwise_fma(ha * u, u, (hd * dy) * dy);
}

// Exact test "can this splat reach alpha >= 1/255 at some pixel centre of the box [x0,x1] x [y0,y1]" (continuous box,
// conservative margins).  alpha >= 1/255  <=>  sigma <= tau = ln(255 o); the x-span of (ellipse 1/2 d^T Q d <= tau) intersected
// with the band dy in [y0-my, y1-my] is [left, right] with right = hx if the ellipse's rightmost point lies in the band, else
// the larger chord end at the band edges (see binning.hip, row_span); the box is reachable iff that span meets [x0, x1].
// The margins absorb the 1-ulp hardware rcp / sqrt and the fp32 rounding of exp / log: a pair the exact per-pixel test would keep
// is never culled; candidates still go through the exact per-pixel test.
__device__ __forceinline__ bool box_reachable(float mx, float my, float a, float b, float c, float opacity,
                                              float x0, float x1, float y0, float y1) {
    const float tau = __logf(255.f * opacity) * 1.0002f + 2e-4f;
    if (!(tau > 0.f)) return false;
    const float det = conic_det(a, b, c);
    if (!(det > 0.f) || !(a > 0.f) || !(c > 0.f)) return true;     // not an ellipse: never cull
    const float two_tau = 2.f * tau;
    const float rdet = __builtin_amdgcn_rcpf(det);
    const float hy = __builtin_amdgcn_sqrtf(two_tau * a * rdet) * 1.0004f + 1e-3f;
    float lo = y0 - my, hi = y1 - my;
    if (hi < -hy || lo > hy) return false;
    lo = fmaxf(lo, -hy); hi = fminf(hi, hy);
    const float tta = two_tau * a;
    const float rlo = __builtin_amdgcn_sqrtf(fmaxf(0.f, tta - det * lo * lo));
    const float rhi = __builtin_amdgcn_sqrtf(fmaxf(0.f, tta - det * hi * hi));
    const float hx = __builtin_amdgcn_sqrtf(two_tau * c * rdet);
    const float dys = b * __builtin_amdgcn_sqrtf(two_tau * rdet * __builtin_amdgcn_rcpf(c));
    const float inv_a = __builtin_amdgcn_rcpf(a);
    const float right = (-dys >= lo && -dys <= hi) ? hx : fmaxf((-b * lo + rlo) * inv_a, (-b * hi + rhi) * inv_a);
    const float left = (dys >= lo && dys <= hi) ? -hx : fminf((-b * lo - rlo) * inv_a, (-b * hi - rhi) * inv_a);
    const float eps = 2e-3f + 5e-4f * hx;
    return (mx + right + eps >= x0) && (mx + left - eps <= x1);
}

// box_reachable for a GRID of boxes of one tile at once: BANDS horizontal bands of 16 / BANDS pixel rows, each cut into a left and
// a right half of 8 pixel columns.  Bit (2 * band + half) of the result = that 8 x (16 / BANDS) box is reachable.  The per-splat
// terms (tau, extents, the tangent offset) are shared, the chord ends are per band.  (tx0, ty0) is the centre of the tile's first
// pixel.  BANDS = 2: the four 8x8 quadrants; BANDS = 4: eight 8x4 units.
template <int BANDS>
__device__ __forceinline__ unsigned band_half_mask(float mx, float my, float a, float b, float c, float opacity, float tx0, float ty0) {
    constexpr float BH = (float)(TILE / BANDS);
    const float tau = __logf(255.f * opacity) * 1.0002f + 2e-4f;
    if (!(tau > 0.f)) return 0u;
    const float det = conic_det(a, b, c);
    if (!(det > 0.f) || !(a > 0.f) || !(c > 0.f)) return (1u << (2 * BANDS)) - 1u;      // not an ellipse: never cull
    const float two_tau = 2.f * tau;
    const float rdet = __builtin_amdgcn_rcpf(det);
    const float hy = __builtin_amdgcn_sqrtf(two_tau * a * rdet) * 1.0004f + 1e-3f;
    const float tta = two_tau * a;
    const float hx = __builtin_amdgcn_sqrtf(two_tau * c * rdet);
    const float dys = b * __builtin_amdgcn_sqrtf(two_tau * rdet * __builtin_amdgcn_rcpf(c));
    const float inv_a = __builtin_amdgcn_rcpf(a);
    const float eps = 2e-3f + 5e-4f * hx;
    unsigned m = 0u;
#pragma unroll
    for (int band = 0; band < BANDS; ++band) {
        const float y0 = ty0 + BH * (float)band;
        float lo = y0 - my, hi = (y0 + (BH - 1.f)) - my;
        if (hi < -hy || lo > hy) continue;
        lo = fmaxf(lo, -hy); hi = fminf(hi, hy);
        const float rlo = __builtin_amdgcn_sqrtf(fmaxf(0.f, tta - det * lo * lo));
        const float rhi = __builtin_amdgcn_sqrtf(fmaxf(0.f, tta - det * hi * hi));
        const float right = (-dys >= lo && -dys <= hi) ? hx : fmaxf((-b * lo + rlo) * inv_a, (-b * hi + rhi) * inv_a);
        const float left = (dys >= lo && dys <= hi) ? -hx : fminf((-b * lo - rlo) * inv_a, (-b * hi - rhi) * inv_a);
        const float xr = mx + right + eps, xl = mx + left - eps;
        if (xr >= tx0 && xl <= tx0 + 7.f) m |= 1u << (2 * band);
        if (xr >= tx0 + 8.f && xl <= tx0 + 15.f) m |= 2u << (2 * band);
    }
    return m;
}

// ---- segmented backward (round 5) -------------------------------------------------------------------------------------------------
// The backward walks a tile's list back to front with one workgroup: in a scene whose lists are heavy-tailed (a trained model: a few
// tiles walk thousands of entries where the median walks a few hundred) the launch lasts as long as its longest tile
// (`synthetic.scene_surfaces`: 0.57 ms against ~0.40 for the same work spread evenly).  The forward therefore leaves a CHECKPOINT of
// every pixel's running state each SEG list entries, and the backward cuts a walk longer than SEG into segments that ANY workgroup
// may process: a pixel that continues beyond a segment's far end starts from the checkpoint there (its transmittance in front of
// that entry, and the colour accumulated from that entry on) instead of from its final state.
//   forward   accumulates the colour PER SEGMENT (the sum restarts at every boundary; the image is the sum of the segment sums) and,
//             when it is done, turns the stored segment sums into suffix sums from the back — small deep contributions are added to
//             each other first, as the backward's own running sum does (a difference "final - prefix" would cancel).
//             ckpt[(p >> SEG_LOG2) * 256 + quadrant * 64 + lane] = (T in front of entry p, colour accumulated from entry p on),
//             p = tile start + k SEG, k >= 1: boundaries of different tiles are more than SEG apart (each lies at least SEG behind
//             its tile's start), so p >> SEG_LOG2 is a collision-free slot index.  It also clears the frame's item counter.
//   backward  two launches: the first is the plain kernel cut to segment 0 of every tile (a walk of at most SEG entries: all of it);
//             a tile with a longer walk PUBLISHES its segments 1.. as work items, and the second launch — one workgroup per item
//             slot (list capacity / SEG: what the host knows) — serves them.  No workgroup waits for another; nothing depends on
//             dispatch order.
//   ADAPTIVE  a frame is segmented only when ITS VIEW's walks have a tail.  Every backward workgroup adds its tile's walk length to a small
//             table of device words (sum, maximum, non-empty tiles; 64 rows by tile index, fire-and-forget atomics); the NEXT frame's
//             forward kernel — behind that backward on the stream, so the table is complete — reduces it, stores a verdict into the slot of
//             a small ring of pinned host words it was given (ticket << 1 | tail; tail = the longest walk exceeds SEG_TRIGGER entries AND
//             4.5 x the mean walk of the non-empty tiles, SEG_TAIL_X2 / 2) and clears the table.  The host — no synchronisation — reads the
//             slots that have landed before a later forward and remembers the verdict PER VIEW (the address of the view matrix the
//             previous frame was rendered with: a data set's cameras are persistent tensors); a frame is segmented when its view's last
//             verdict was "tail", a view without a verdict follows the stream (segmented for 64 frames after any "tail").
//             Measured per view (profiles/r23_walk_tail_probe.txt): with a longest walk above 768 the plain kernel wins by 44-61 us up
//             to a ratio of 3.3, the segmented form by 43-960 us from 5.6 on — every view of a trained-scene-shaped frame, and ONE far
//             view of the metric workload's heterogeneous set (-131 us), which a per-stream switch could not take without dragging the
//             fifteen views that lose 14-61 us along.  (Round 5's trigger was the length alone: close-up views of the uniform cloud walk
//             800-1000 entries in EVERY tile — no tail, nothing to spread — and paid 38 us for checkpoints and a second launch.)
// D == 3 (a checkpoint is one float4), and D == 4 in the Inria mode (the fused call's inverse-depth channel, GSPL_INRIA_INVDEPTH: the
// float4 holds T and the three colours, `ckpt_x` — same slot index, one float — the 4th channel); off (ckpt == nullptr) everywhere else.
#ifndef GSPL_SEG_LOG2
#define GSPL_SEG_LOG2 8      // 256 entries per segment (measured on scene_surfaces, per step: 64 -> 1.63 ms, 128 -> 1.45, 256 -> 1.47, 512 -> 1.56, 1024 -> 1.72;
                             // 128 costs the forward 4 % more for its checkpoints and twice the checkpoint memory: profiles/r07v_segment_sizes.txt)
#endif
static constexpr int SEG_LOG2 = GSPL_SEG_LOG2;
static constexpr int SEG = 1 << SEG_LOG2;
static constexpr int SEG_TRIGGER = 3 * SEG;    // a walk longer than this (and SEG_TAIL x the mean walk) switches the segmented form on (a tile of two segments is not worth a second launch)
static constexpr int SEG_TAIL_X2 = 9;          // ... the launch lasts as long as its longest tile only when that tile is far longer than the bulk: 2 x longest > 9 x mean
static constexpr int SEG_WALK_SLOTS = 64;      // rows of (sum, max, non-empty tiles, -) in SegState::walk
static constexpr int SEG_MAX = 255;            // segments per tile (8 bits in a work item); the last one takes whatever is left
struct SegState {
    float4* ckpt;
    uint32_t* words;      // [0]: published work items (zero before the backward); [2 .. 2 + slots): the items, (tile << 8) | segment
    uint32_t* host_flag;  // pinned host word (a slot of the verdict ring): receives (ticket << 1) | "the last backward's walks had a tail" (nullable)
    uint32_t ticket;      // ... of this forward
    uint32_t* walk;       // device, [SEG_WALK_SLOTS][4]: the backward's walk statistics, reduced and cleared by the next forward (nullable)
    uint4* zero_p;        // forward only: a block this launch clears on behalf of the backward (its packed rows: GSPL_BUF_PACKED), 16-byte units
    uint32_t zero_n16;
    uint32_t slots;
    float* ckpt_x;        // D == 4: the 4th channel of every checkpoint (indexed as ckpt); nullptr with D == 3
    __host__ __device__ uint32_t* count() const { return words; }
    __host__ __device__ uint32_t* work() const { return words + 2; }
};

__device__ __forceinline__ void tile_range(int tile, int n_tiles, int64_t n_isects,
                                           const int32_t* __restrict__ offsets, int& start, int& end) {
    start = offsets[tile];
    // n_isects < 0: `offsets` has n_tiles + 1 entries, the last one is the list length (device-side count, gspl_bin_sort_device_count)
    end = (tile + 1 < n_tiles || n_isects < 0) ? offsets[tile + 1] : (int)n_isects;
}

// The tile lists may be cut on 8-, 16- or 32-pixel tiles (`tile_size` of the callers: gsplat_v1_renderer.py:23-41); the kernels
// always work on 8x8 pixel blocks grouped into 16x16 compute tiles.  The list of a block is the list of the LIST tile that holds it.
struct ListTiles {
    int log2;      // list tile side = 1 << log2 (3, 4, 5)
    int w;         // list tiles per row
    int n;         // number of list tiles
};
static inline ListTiles list_tiles(TileGrid grid) {
    ListTiles lt;
    lt.log2 = grid.size == 8 ? 3 : (grid.size == 32 ? 5 : 4);
    lt.w = grid.w;
    lt.n = grid.n();
    return lt;
}
// ... and the 16x16 compute grid of an image: what the kernels' `tile_w` and `n_tiles` are, whatever the lists were cut on
struct ImageSize { int width, height; };
struct ComputeTiles { int w, n; };
static inline ComputeTiles compute_tiles(ImageSize image) {
    const int w = (image.width + TILE - 1) / TILE;
    return ComputeTiles{w, w * ((image.height + TILE - 1) / TILE)};
}
__device__ __forceinline__ void block_list_range(const ListTiles& lt, int bx, int by, int width, int height, int64_t n_isects,
                                                 const int32_t* __restrict__ offsets, int& start, int& end) {
    if (bx * 8 >= width || by * 8 >= height) { start = end = 0; return; }      // (a block of the compute grid outside the image)
    const int t = (by >> (lt.log2 - 3)) * lt.w + (bx >> (lt.log2 - 3));
    start = offsets[t];
    end = (t + 1 < lt.n || n_isects < 0) ? offsets[t + 1] : (int)n_isects;
}

// ---- the 8x8 block walk -----------------------------------------------------------------------------------------------------------
// One wave per 8x8 pixel block, one pixel per lane, the block's list in rounds of 64 entries: composite_fwd_kernel and
// composite_scores_kernel (composite.hip), composite_bwd_block_kernel (composite_bwd.hip), feature_fwd_kernel and feature_bwd_kernel
// (features.hip).  The kernels must take the same discrete decisions bit for bit (the hit flags equal `count > 0` of the statistics
// pass, the wide-feature image equals the narrow kernels', a backward re-derives the pairs its forward blended), so the block, the
// round, the per-pixel alpha and the blending decision are defined here once.  What a kernel keeps to itself: where its list comes
// from (block_list_range or tile_range) and in which direction it walks it, what it stages per candidate beside the six common
// arrays, and what it does with a blended pair.  composite_bwd2_kernel (two pixels per lane, band_half_mask) has its own packed walk.
struct WalkBlock {
    int bx, by, w;                    // the block in units of 8 pixels; w: its quadrant of the 16x16 compute tile
    int px, py;                       // this lane's pixel
    float pxf, pyf;                   // ... and its centre
    float qx0, qx1, qy0, qy1;         // the block's pixel-centre bounds (wave-uniform)
};
// unit = 4 * compute tile + quadrant; tile_w: compute tiles per row
template <int MODE>
__device__ __forceinline__ WalkBlock walk_block(int unit, int tile_w) {
    using TR = ModeTraits<MODE>;
    WalkBlock b;
    const int tile = unit >> 2, l = threadIdx.x;
    b.w = unit & 3;
    b.bx = (tile % tile_w) * 2 + (b.w & 1); b.by = (tile / tile_w) * 2 + (b.w >> 1);
    b.px = b.bx * 8 + (l & 7); b.py = b.by * 8 + (l >> 3);
    b.pxf = (float)b.px + TR::kPixelCentre; b.pyf = (float)b.py + TR::kPixelCentre;
    b.qx0 = (float)(b.bx * 8) + TR::kPixelCentre; b.qx1 = b.qx0 + 7.f;
    b.qy0 = (float)(b.by * 8) + TR::kPixelCentre; b.qy1 = b.qy0 + 7.f;
    return b;
}

// One round's candidates in LDS, structure of arrays: centre, sigma_coef, opacity.  `__shared__ RoundLists s;`
struct RoundLists { float x[64], y[64], ha[64], k[64], hd[64], op[64]; };
struct RoundSlot {
    int ncand;        // candidates of the round (wave-uniform)
    int slot;         // this lane's candidate goes to slot `slot`, if `cand`: the number of candidates in lower lanes, so the slots
    bool cand;        // follow the lanes' order whichever way the caller walks its list
    float b, c;       // the conic's b and c as this lane loaded them
};
// Lane l holds one list entry (`has`: there is one; g: its splat), tests it against the block and the survivors' common fields land in
// slots 0 .. ncand - 1.  The caller stages what else it needs at r.slot and then closes the round with a barrier of its own: a wave
// barrier, or __syncthreads() in a one-wave workgroup.  (composite_fwd_kernel keeps its own copy of this: its arrays carry a padding
// entry for the packed loop, its colours are staged with the gather, and it runs without wave barriers.  Built on this helper — arrays
// of 66, no barrier — its D = 3 instantiations go from 42 / 56 to 43 / 58 VGPRs: profiles/block_walk_kernel_resources.txt.)
__device__ __forceinline__ RoundSlot compact_round(bool has, int g, const float* __restrict__ means2d, const float* __restrict__ conics,
                                                   const float* __restrict__ opacities, const WalkBlock& b, RoundLists& s) {
    RoundSlot r;
    r.cand = false;
    float mx = 0.f, my = 0.f, ca = 0.f, op = 0.f;
    r.b = r.c = 0.f;
    if (has) {
        ca = conics[g * 3 + 0]; r.b = conics[g * 3 + 1]; r.c = conics[g * 3 + 2]; op = opacities[g];
        mx = means2d[g * 2 + 0]; my = means2d[g * 2 + 1];
        r.cand = box_reachable(mx, my, ca, r.b, r.c, op, b.qx0, b.qx1, b.qy0, b.qy1);
    }
    const unsigned long long mask = __ballot(r.cand);
    r.ncand = __builtin_popcountll(mask);
    r.slot = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    __builtin_amdgcn_wave_barrier();
    if (r.cand) {
        const SigmaCoef sc = sigma_coef(ca, r.b, r.c);
        s.x[r.slot] = mx; s.y[r.slot] = my; s.ha[r.slot] = sc.ha; s.k[r.slot] = sc.k; s.hd[r.slot] = sc.hd; s.op[r.slot] = op;
    }
    return r;
}

// Candidate k at the pixel centre (pxf, pyf): sigma and the unclamped opacity * exp(-sigma).  Each component of the packed loops of
// composite_fwd_kernel and composite_bwd2_kernel (eval_sigma2, exp2 of sigma * -log2 e) is this expression tree.
struct PixelAlpha { float dx, dy, sigma, raw; };
__device__ __forceinline__ PixelAlpha pixel_alpha(const RoundLists& s, int k, float pxf, float pyf) {
    PixelAlpha a;
    a.dx = s.x[k] - pxf; a.dy = s.y[k] - pyf;
    a.sigma = eval_sigma(s.ha[k], s.k[k], s.hd[k], a.dx, a.dy);
    a.raw = s.op[k] * __builtin_amdgcn_exp2f(a.sigma * -1.4426950408889634f);
    return a;
}
template <int MODE>
__device__ __forceinline__ float clamp_alpha(float raw) { return fminf(ModeTraits<MODE>::kAlphaMax, raw); }

// "this pixel takes this splat" (alpha clamped or not: kAlphaMax > 1/255).  `live`: the forward's "not done", a backward's "not behind
// the pixel's last contributor" — an operand here and not `live && alpha_test(..)` at the callers: that associates the three conditions
// the other way round, and hipcc then schedules composite_fwd_kernel's inner loop differently (profiles/block_walk_ab.txt).
__device__ __forceinline__ bool alpha_test(bool live, float sigma, float alpha) { return live && (sigma >= 0.f) && (alpha >= kAlphaMin); }

// The forward's blending decision for one (pixel, candidate): returns whether the pair is blended, `wgt` = its weight alpha T (0 if
// not), and moves T and `done` on.  A pixel stops IN FRONT of the splat that would take its transmittance below 1e-4.
template <int MODE>
__device__ __forceinline__ bool blend_step(float sigma, float alpha, float& T, bool& done, float& wgt) {
    const bool valid = alpha_test(!done, sigma, alpha);
    const float next_T = T * (1.f - alpha);
    const bool stop = valid && (ModeTraits<MODE>::kStopInclusive ? (next_T <= kTStop) : (next_T < kTStop));
    const bool contrib = valid && !stop;
    wgt = contrib ? alpha * T : 0.f;
    T = contrib ? next_T : T;
    done = done || stop;
    return contrib;
}

// A table of float arrays to clear, and the grid that clears it: `blocks` workgroups of NT threads each, workgroup `block` of them.
// Streaming stores (the arrays are read again only by the kernels behind the one that clears them); per array the floats in front of
// the first 16-byte boundary, 16-byte chunks, the floats behind the last one.  Runs as a launch of its own (zero_fill_kernel, fused.hip)
// or as the role of the first `blocks` workgroups of composite_bwd2_kernel<.., FILL = true>.
struct FillJob {
    struct Span { float* p; uint64_t n; } a[9];      // n: floats
    int count = 0;
    int blocks = 0;
    void add(float* p, uint64_t n) { if (p && n) a[count++] = Span{p, n}; }
};
template <int NT>
__device__ __forceinline__ void zero_fill_body(const FillJob& job, unsigned block, unsigned blocks) {
    const uint64_t tid = (uint64_t)block * NT + threadIdx.x, stride = (uint64_t)blocks * NT;
    for (int k = 0; k < job.count; ++k) {
        float* p = job.a[k].p;
        const uint64_t n = job.a[k].n;
        const uint64_t head = min(n, (uint64_t)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2));
        const uint64_t n4 = (n - head) >> 2, tail0 = head + (n4 << 2);
        for (uint64_t i = tid; i < n4; i += stride) store16_nt(p + head, i, make_float4(0.f, 0.f, 0.f, 0.f));
        if (tid < head) p[tid] = 0.f;
        if (tid < n - tail0) p[tail0 + tid] = 0.f;
    }
}

// number of per-splat gradient values accumulated per (tile, splat): xy(2) conic(3) opacity(1) colour(D) [+abs xy(2)]
template <int D, bool ABS> struct BwdVals { static constexpr int N = 6 + D + (ABS ? 2 : 0); };

// argument groups of the compositing calls below the ABI (gspl_host.h has the tile grid; ImageSize: above): the splats as compositing
// reads them, and the per-tile lists (n_isects < 0: `offsets` has one more entry, the list length, left there by the device)
struct CompositeSplats { const float* means2d; const float* conics; const float* colors; const float* opacities; const float* backgrounds; };
struct TileLists { const int32_t* offsets; const int32_t* flatten_ids; int64_t n_isects; };

int check_composite_args(int N, int64_t n_isects, int D, int mode, int layout, ImageSize image, TileGrid grid, const char* who);

// gspl_composite_fwd / gspl_composite_bwd_packed with the segmentation state of the fused Inria call (fused.hip); seg == NULL: off
int composite_fwd_impl(int N, int D, int mode, int layout, const CompositeSplats& splats, ImageSize image, TileGrid grid, const TileLists& lists,
                       float* out_colors, float* out_alphas, float* final_Ts, int32_t* last_ids, uint8_t* hit_flags, void* stream, const SegState* seg);
// `fill` (fused.hip, the sparse tail of the Inria backward; NULL everywhere else): arrays to clear, by fill->blocks extra workgroups at
// the FRONT of the first composite_bwd2_kernel launch.  Needs the Inria mode, CHW, D 3 or 4, 16-pixel list tiles, no absgrad.
int composite_bwd_packed_impl(int N, int D, int mode, int layout, const CompositeSplats& splats, ImageSize image, TileGrid grid, const TileLists& lists,
                              const float* final_Ts, const int32_t* last_ids, const float* v_out_colors, const float* v_out_alphas,
                              float* v_packed, int packed_stride, int absgrad, uint8_t* hit_flags, void* stream, const SegState* seg,
                              const FillJob* fill = nullptr);

// One launch of a kernel family templated on <D, MODE, CHW>: f(D, MODE, CHW) gets the three as std::integral_constants and returns the
// call's code.  check_composite_args has refused every other mode and layout; a D outside {1, 2, 3, 4, 8} is GSPL_ERR_UNSUPPORTED.
template <class F>
static int dispatch_composite(int D, int mode, int layout, F&& f) {
    auto with_d = [&](auto mode_c, auto chw_c) -> int {
        return dispatch_int<1, 2, 3, 4, 8>(D, [&](auto d) -> int { return f(d, mode_c, chw_c); }, (int)GSPL_ERR_UNSUPPORTED);
    };
    return dispatch_bools([&](auto inria, auto chw) { return with_d(std::integral_constant<int, decltype(inria)::value ? GSPL_MODE_INRIA : GSPL_MODE_GSPLAT>{}, chw); },
                          mode != GSPL_MODE_GSPLAT, layout != GSPL_LAYOUT_HWC);
}

// The deterministic mode's ordered reduction (composite_bwd.hip; gspl_set_deterministic): a backward that wrote one row of `nv` (<= 18)
// floats per list entry adds, per splat, its entries' rows IN LIST ORDER into rows[splat * row_stride ...] (which the caller cleared,
// or filled with what the sums are added to).  One block of ordered_scratch(...).total bytes, carved as entries | four key arrays | the
// sort's workspace: it starts with the entries' rows, which the caller clears before the backward that fills them.
struct OrderedScratch { size_t keys, sort_ws, sort_ws_bytes, total; int id_bits; };
OrderedScratch ordered_scratch(int N, int64_t n_isects, int nv);
int ordered_reduce(int N, int64_t n_isects, int nv, const int32_t* flatten_ids, void* block, float* rows, int row_stride, hipStream_t s, const char* who);

}  // namespace gspl

/*
 * gspl_hip.h — C ABI of the MI355X (gfx950) Gaussian-splatting rasterizer hot path.
 *
 * This is the drop-in boundary: every entry point takes raw device
 * pointers + sizes + a hipStream_t passed as void*, returns an int status
 * (GSPL_OK == 0) and never throws.  No torch types cross this line; the Python
 * host side (gaussian-splatting-lightning_amd/ops/) binds it with ctypes and
 * allocates every buffer through torch's caching allocator.
 *
 * Each function names the reference interface it replaces.  Paths are relative to
 * the reference tree (yzslab/gaussian-splatting-lightning); the native ops the
 * reference calls live in un-vendored third-party CUDA packages
 * (gsplat @ yzslab/gsplat c27a44d4, diff_gaussian_rasterization @ 59f5f77e), so the
 * citations are the reference's *call sites* of those ops.
 *
 * Conventions
 *   - all arrays are dense, row-major, fp32 unless stated; "i32"/"i64"/"u8" stated.
 *   - quaternions are (w,x,y,z) and are used as given (the reference hands over
 *     normalised rotations: internal/models/vanilla_gaussian.py:357-358,
 *     internal/utils/gaussian_projection.py:211-232).
 *   - `mode` selects the per-API constants:
 *       GSPL_MODE_GSPLAT : pixel centre at +0.5, alpha <= 0.999, stop when T(1-a) <= 1e-4,
 *                          clamped alpha has zero gradient, tile rect [floor, floor+1)
 *       GSPL_MODE_INRIA  : pixel centre at integers, alpha <= 0.99, stop when T(1-a) < 1e-4,
 *                          clamp ignored in backward, tile rect [(p-r)/T, (p+r+T-1)/T)
 *   - nullable pointers are marked; a NULL optional output is simply not written.
 */
#ifndef GSPL_HIP_H
#define GSPL_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes */
enum {
    GSPL_OK = 0,
    GSPL_ERR_INVALID_ARG = 1,   /* bad size / NULL required pointer / unsupported channel count */
    GSPL_ERR_WORKSPACE = 2,     /* caller-provided workspace too small */
    GSPL_ERR_LAUNCH = 3,        /* hipGetLastError() != hipSuccess after a launch */
    GSPL_ERR_UNSUPPORTED = 4
};

enum { GSPL_MODE_GSPLAT = 0, GSPL_MODE_INRIA = 1 };

/* camera model of gspl_project_fwd/bwd (gsplat v1 `camera_model`, reference option internal/renderers/gsplat_v1_renderer.py:50) */
enum { GSPL_CAMERA_PINHOLE = 0, GSPL_CAMERA_ORTHO = 1, GSPL_CAMERA_FISHEYE = 2 };

/* image memory layout of composite outputs / incoming image gradients */
enum { GSPL_LAYOUT_HWC = 0, GSPL_LAYOUT_CHW = 1 };

/* ABI version, bumped on any signature change; checked by the ctypes loader. */
#define GSPL_ABI_VERSION 39
int gspl_abi_version(void);
/* Human-readable description of the last launch error on this thread (never NULL). */
const char* gspl_last_error(void);

/* ------------------------------------------------------------------------------------------
 * 1. Projection (EWA splatting): 3D mean/scale/rotation -> 2D mean, depth, conic, radius.
 *    Replaces gsplat `fully_fused_projection` (internal/renderers/gsplat_v1_renderer.py:408-421,
 *    gsplat_distributed_renderer.py:271-283) and gsplat-v0 `project_gaussians`
 *    (gsplat_renderer.py:64-79); math pinned to internal/utils/gaussian_projection.py:6-138.
 *    One thread per (camera, Gaussian); C cameras batched.
 *      viewmats [C,4,4]  world->camera, standard (non-transposed) row-major, device memory
 *      Ks       [C,3,3]  intrinsics, device memory
 *    Outputs (all [C,N,...]): radii i32 (0 = culled), means2d [.,2], depths, conics [.,3],
 *    compensations (nullable), tiles_hit i32 (nullable; v0 `num_tiles_hit`), cov3d [.,6] (nullable): the upper triangle
 *    (xx, xy, xz, yy, yz, zz) of Sigma = (R S)(R S)^T that `project_gaussians` returns as `cov3d` (gaussian_projection.py:47,137).
 *    Culled Gaussians get zeros in every output (gaussian_projection.py:127-136).
 *    camera_model: GSPL_CAMERA_PINHOLE is the in-tree Python above (1.3 tan(fov) clamp of the Jacobian's x/z, y/z).
 *    GSPL_CAMERA_ORTHO / GSPL_CAMERA_FISHEYE (the `camera_model` option the reference passes through,
 *    gsplat_v1_renderer.py:50,154) restate the published gsplat models — ortho: mean2d = (fx x + cx, fy y + cy),
 *    J = diag(fx, fy) | 0; fisheye (equidistant): mean2d = f * (x, y) * atan2(r, z) / r + c with the closed-form Jacobian —
 *    without the clamp; everything after the 2D covariance (low-pass, radius, rect, culling) is shared.
 * ---------------------------------------------------------------------------------------- */
int gspl_project_fwd(int C, int N,
                     const float* means, const float* scales, const float* quats,
                     const float* viewmats, const float* Ks,
                     int width, int height, int tile_size,
                     float scale_modifier, float eps2d, float near_plane, float far_plane,
                     float radius_clip, int camera_model,
                     int32_t* radii, float* means2d, float* depths, float* conics,
                     float* compensations /*nullable*/, int32_t* tiles_hit /*nullable*/, float* cov3d /*nullable*/,
                     void* stream);

/*    Backward of the above (autograd of gsplat's op; reference enters it through
 *    `manual_backward`, internal/gaussian_splatting.py:380).  v_means/v_scales/v_quats are
 *    OVERWRITTEN when C == 1 and must be zero-initialised by the caller when C > 1
 *    (accumulated with atomics across cameras).  v_compensations / v_depths nullable.  The strides let the
 *    columns of gspl_composite_bwd_packed's row buffer be consumed in place (C == 1 only). */
int gspl_project_bwd(int C, int N,
                     const float* means, const float* scales, const float* quats,
                     const float* viewmats, const float* Ks,
                     int width, int height,
                     float scale_modifier, float eps2d, int camera_model,
                     const int32_t* radii,
                     const float* v_means2d, int v_means2d_stride /* floats per row; 0 = dense [.,2] */,
                     const float* v_depths /*nullable = 0*/,
                     const float* v_conics, int v_conics_stride /* 0 = dense [.,3] */,
                     const float* v_compensations /*nullable*/,
                     float* v_means, float* v_scales, float* v_quats,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * 2. Spherical harmonics -> colour.
 *    Replaces gsplat `spherical_harmonics` / `spherical_harmonics_decomposed`
 *    (gsplat_renderer.py:105, gsplat_v1_renderer.py:121-130, gsplat_distributed_renderer.py:416-421);
 *    basis pinned to internal/utils/sh_utils.py:57-171.
 *    Coefficient k of Gaussian n, channel c:
 *        k == 0 : dc  [n*dc_stride   + c]
 *        k >= 1 : rest[n*rest_stride + (k-1)*3 + c]
 *    so the merged [N,K,3] tensor is (dc=base, rest=base+3, both strides 3K) and the decomposed
 *    model storage (shs_dc [N,1,3], shs_rest [N,K-1,3]) is (3, 3(K-1)).
 *    dirs [N,3] need not be normalised (normalised in-kernel, as gsplat does); if `origin`
 *    (device [3], nullable) is given, the direction is dirs[n] - origin (dirs = means).
 *    mask u8 [N] nullable (0 -> colour 0, no gradient).
 *    flags bit0: add 0.5 and clamp at 0 (gsplat_renderer.py:106) inside the kernel;
 *    clamped u8 [N,3] (nullable) then records which channels were clamped (needed by bwd).
 * ---------------------------------------------------------------------------------------- */
enum { GSPL_SH_ADD_HALF_CLAMP = 1 };
int gspl_sh_fwd(int N, int degree,
                const float* dirs, const float* origin /*nullable*/,
                const float* dc, int dc_stride, const float* rest, int rest_stride,
                const uint8_t* mask /*nullable*/, int flags,
                float* colors, uint8_t* clamped /*nullable*/,
                void* stream);
/*    v_dc / v_rest are written with the same strides (every coefficient of every Gaussian is
 *    written, zeros above the active degree / for masked rows, n_coeffs = number of coefficient
 *    rows present per Gaussian); v_dirs [N,3] nullable (gradient w.r.t. dirs, i.e. w.r.t. means
 *    when origin is used — the Inria path needs it, gsplat paths detach: gsplat_renderer.py:104).
 *    A row stride may be larger than the coefficients need; the backward then also writes 0 into the
 *    columns between the last coefficient and the row stride of every v_rest row (of every merged row
 *    when rest == dc + 3), so a caller must not keep other data there (a separate v_dc row gets its
 *    three floats and nothing else). */
int gspl_sh_bwd(int N, int degree, int n_coeffs,
                const float* dirs, const float* origin /*nullable*/,
                const float* dc, int dc_stride, const float* rest, int rest_stride,
                const uint8_t* mask /*nullable*/, int flags, const uint8_t* clamped /*nullable*/,
                const float* v_colors, int v_colors_stride /* floats per row; 0 = dense [N,3] */,
                float* v_dc, float* v_rest, float* v_dirs /*nullable*/,
                void* stream);

/* C cameras in ONE launch — what the Gaussian-sharded renderer needs per step (every rank evaluates its shard for all W
 * cameras: gsplat_distributed_renderer.py:252-311,416-421, a Python loop of W SH calls there).  The coefficient rows are
 * read once for all cameras; colours = clamp(SH(means - origins[c]) + 0.5, 0) with flags = GSPL_SH_ADD_HALF_CLAMP.
 *    means [N,3]; origins [C,3]; radii [C,N] i32 nullable (rows with radius <= 0 are skipped and get zeros);
 *    colors [C,N,3]; clamped [C,N,3] u8 (nullable without the clamp flag).
 * Backward: v_colors [C,N,3] dense -> v_dc / v_rest (same layouts as gspl_sh_bwd) summed over the cameras and written
 * once; no direction gradient (the reference detaches the means here). */
int gspl_sh_fwd_batched(int C, int N, int degree,
                        const float* means, const float* origins,
                        const float* dc, int dc_stride, const float* rest, int rest_stride,
                        const int32_t* radii /*nullable*/, int flags,
                        float* colors, uint8_t* clamped /*nullable*/, void* stream);
int gspl_sh_bwd_batched(int C, int N, int degree, int n_coeffs,
                        const float* means, const float* origins,
                        int dc_stride, int rest_stride,
                        const int32_t* radii /*nullable*/, int flags, const uint8_t* clamped /*nullable*/,
                        const float* v_colors, float* v_dc, float* v_rest, void* stream);

/* ------------------------------------------------------------------------------------------
 * 3. Tile binning: (tile, depth) keys, radix sort, per-tile ranges.
 *    Replaces gsplat `isect_tiles` + `isect_offset_encode` (gsplat_v1_renderer.py:446-458) and
 *    the binning half of v0 `rasterize_gaussians` (gsplat_renderer.py:86-99); key layout pinned
 *    to internal/utils/gaussian_projection.py:159-208: key = (tile_id << 32) | bits(depth),
 *    tile_id row-major, value = Gaussian index.  Single camera per call.
 *
 *    Step a: per-Gaussian tile counts + inclusive prefix sum (i64; block sums, scan of the sums, per-block scan).  Host reads cum[N-1].
 *    Step b: emit keys, sort them (stable LSD radix, so equal-depth ties keep Gaussian order).
 *    Step c: offsets[t] = first sorted index whose tile id is >= t   (t in [0, tiles)).
 *    gspl_isect_workspace_bytes gives the scratch size for steps a and b.
 * ---------------------------------------------------------------------------------------- */
size_t gspl_isect_workspace_bytes(int N, int64_t n_isects);
int gspl_isect_count(int N, int mode,
                     const float* means2d, const int32_t* radii,
                     int tile_size, int tile_w, int tile_h,
                     int32_t* tiles_per_gauss, int64_t* cum_tiles,
                     void* workspace, size_t workspace_bytes, void* stream);
int gspl_isect_emit_sort(int N, int mode,
                         const float* means2d, const int32_t* radii, const float* depths,
                         const int64_t* cum_tiles,
                         int tile_size, int tile_w, int tile_h, int64_t n_isects,
                         int64_t* isect_ids, int32_t* flatten_ids,
                         void* workspace, size_t workspace_bytes, void* stream);
int gspl_isect_offsets(int64_t n_isects, const int64_t* isect_ids,
                       int tile_w, int tile_h, int32_t* offsets, void* stream);

/*    3b. The same binning for callers that only need the per-tile lists (flatten_ids + offsets), not
 *    the 64-bit keys: the fused Inria rasterizer (vanilla_renderer.py:111-120) and gsplat-v0
 *    `rasterize_gaussians` (gsplat_renderer.py:86-99) never see isect_ids.  Two-level, "depth first":
 *    sort the N splats by depth (32-bit keys), emit tile hits in that order, stable-sort by tile id
 *    only.  Produces exactly the flatten_ids / offsets of steps a-c above at a third of the traffic.
 *      order [N] i32 (splat ids by depth, tile-less splats last), cum_tiles [N] i64 (inclusive prefix
 *      sum of tile counts in that order; host reads cum_tiles[N-1]).
 *    conics [N,3] + opacities [N] (both nullable, together): when given, a (tile, splat) pair is listed
 *    only if the splat can reach alpha >= 1/255 somewhere in the tile (exact ellipse-vs-tile test with a
 *    conservative margin).  The dropped pairs contribute nothing to any pixel, so composited images and
 *    gradients are unchanged, while the lists shrink by ~40 % (the 3-sigma square of the reference's
 *    rect is loose, the more so for low opacities).  Pass the SAME opacities the compositing call uses.
 *    spans: caller-owned scratch of GSPL_BIN_SPAN_BYTES per splat, written by gspl_bin_count (the reachable tile
 *    columns of each tile row of the splat: N records for rows 0..7, then N records for rows 8..15 that only taller
 *    splats touch) and read back, in depth order, by gspl_bin_emit_sort — one 32-byte line per splat instead of
 *    re-gathering means2d / radii / conics / opacities at random addresses.
 * ---------------------------------------------------------------------------------------- */
enum { GSPL_BIN_SPAN_BYTES = 64 };
size_t gspl_bin_workspace_bytes(int N, int64_t n_isects);
int gspl_bin_count(int N, int mode,
                   const float* means2d, const int32_t* radii, const float* depths,
                   const float* conics /*nullable*/, const float* opacities /*nullable*/,
                   int tile_size, int tile_w, int tile_h,
                   int32_t* order, int64_t* cum_tiles /* [N + 1]: inclusive scan of the tile counts in depth order, then
                                                         n_big = the number of splats spanning more than 16 tile rows
                                                         (radius > ~128 px: close-ups, sky blobs) or with a very wide row */,
                   int32_t* big_list /* [N]: the depth-order indices of those splats (n_big entries, ranked by the scan);
                                        the emission deals them out to its workgroups instead of leaving up to 64
                                        consecutive screen-filling splats to one wave */,
                   void* spans /* GSPL_BIN_SPAN_BYTES * N, 16-byte aligned */,
                   int64_t* host_counts /* nullable: two int64 of device-accessible HOST memory (hipHostMalloc / a pinned tensor);
                                           the last kernel stores cum_tiles[N-1] (the list length) and n_big there itself, so a
                                           host that records an event after this call and waits for it needs no copy */,
                   void* workspace, size_t workspace_bytes, void* stream);
int gspl_bin_emit_sort(int N, int mode,
                       const float* means2d, const int32_t* radii,
                       const float* conics /*nullable*/, const float* opacities /*nullable*/,
                       const int32_t* order, const int64_t* cum_tiles, const int32_t* big_list, const void* spans,
                       int tile_size, int tile_w, int tile_h, int64_t n_isects,
                       int32_t* flatten_ids, int32_t* offsets,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The two halves of gspl_bin_emit_sort, so that the emission can be launched SPECULATIVELY while the host still waits
 * for the list length: `capacity` (>= the length, if the guess is good) sizes the workspace
 * (gspl_bin_workspace_bytes(N, capacity)); records past it are dropped.  gspl_bin_sort then takes the real
 * n_isects <= capacity; when the guess was too low the caller repeats gspl_bin_emit with capacity = n_isects. */
int gspl_bin_emit(int N, int mode, const float* means2d, const int32_t* radii,
                  const float* conics /*nullable*/, const float* opacities /*nullable*/,
                  const int32_t* order, const int64_t* cum_tiles, const int32_t* big_list, const void* spans,
                  int tile_size, int tile_w, int tile_h, int64_t capacity,
                  void* workspace, size_t workspace_bytes, void* stream);
int gspl_bin_sort(int N, int tile_w, int tile_h, int64_t n_isects, int64_t capacity,
                  int32_t* flatten_ids, int32_t* offsets, void* workspace, size_t workspace_bytes, void* stream);
/* The same for a host that has not read the list length back yet: it stays on the device (n_isects_dev = &cum_tiles[N - 1]), the
 * sort's grid is sized by `capacity`.  flatten_ids: room for `capacity` ids; offsets: tile_w * tile_h + 1 entries, the last one
 * receives the list length — the compositing entry points take n_isects = -1 with such an array.  The caller compares the
 * length with `capacity` once it has it (gspl_bin_count's host_counts) and repeats emission and sort when the guess was too low. */
int gspl_bin_sort_device_count(int N, int tile_w, int tile_h, const int64_t* n_isects_dev, int64_t capacity,
                               int32_t* flatten_ids, int32_t* offsets, void* workspace, size_t workspace_bytes, void* stream);
/* Sorts and scans of this library are in-tree kernels (csrc/sort.hip): every radix pass is count -> digit-row scan -> scatter
 * over contiguous tile ranges, the scans are block sums -> scan of the sums -> per-block scan.  No workgroup waits for another,
 * so they make progress under any dispatch order and contention, and their output is bit-reproducible. */

/* ------------------------------------------------------------------------------------------
 * 4. Tile compositing, forward.
 *    Replaces gsplat `rasterize_to_pixels` (gsplat_v1_renderer.py:588-601), v0
 *    `rasterize_gaussians` (gsplat_renderer.py:86-99, pypreprocess_gsplat_renderer.py:45-58) and
 *    the render stage of the Inria `GaussianRasterizer` (vanilla_renderer.py:111-120).
 *    One 16x16 tile per workgroup (4 wave64), front-to-back.
 *      colors [N,D], D in {1,2,3,4,8}; backgrounds [D] nullable (treated as 0)
 *      offsets [tile_h*tile_w] i32, flatten_ids [n_isects] i32
 *    Outputs: out_colors ([H,W,D] or [D,H,W] by `layout`), out_alphas [H,W] (= 1 - T_final),
 *             final_Ts [H,W] (the final transmittance itself: backward divides by it, and
 *             1 - (1 - T) in fp32 would lose up to 6e-4 relative at T ~ 1e-4),
 *             last_ids [H,W] i32 (one past the index into flatten_ids of the last contributor;
 *             the tile's range start when the pixel has none).
 * ---------------------------------------------------------------------------------------- */
int gspl_composite_fwd(int N, int64_t n_isects, int D, int mode, int layout,
                       const float* means2d, const float* conics, const float* colors,
                       const float* opacities, const float* backgrounds /*nullable*/,
                       int width, int height, int tile_size, int tile_w, int tile_h,
                       const int32_t* offsets, const int32_t* flatten_ids,
                       float* out_colors, float* out_alphas, float* final_Ts, int32_t* last_ids,
                       uint8_t* hit_flags /*nullable: [N], zeroed by the caller; 1 = some pixel composited the splat (the
                                            fork's has_hit_any_pixels / acc_vis, gsplat_v1_renderer.py:287)*/,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * 5. Tile compositing, backward (the graded kernel: SURVEY.md §8 a12).
 *    Back-to-front per pixel from last_ids; gradients are reduced over the 64 pixels of a wave
 *    with DPP, then over the 4 waves of the tile in LDS, then one fp32 L2 atomic per value per
 *    (tile, Gaussian).  All v_* outputs must be zero-initialised by the caller.
 *      v_out_colors laid out like out_colors; v_out_alphas [H,W] nullable.
 *      v_means2d_abs [N,2] nullable (gsplat `absgrad`, vanilla_density_controller.py:112-113).
 * ---------------------------------------------------------------------------------------- */
int gspl_composite_bwd(int N, int64_t n_isects, int D, int mode, int layout,
                       const float* means2d, const float* conics, const float* colors,
                       const float* opacities, const float* backgrounds /*nullable*/,
                       int width, int height, int tile_size, int tile_w, int tile_h,
                       const int32_t* offsets, const int32_t* flatten_ids,
                       const float* final_Ts, const int32_t* last_ids,
                       const float* v_out_colors, const float* v_out_alphas /*nullable*/,
                       float* v_means2d, float* v_means2d_abs /*nullable*/,
                       float* v_conics, float* v_colors, float* v_opacities,
                       uint8_t* hit_flags /*nullable: u8 [N], zero-initialised; set to 1 for every splat that some pixel
                                            composited (alpha >= 1/255 before termination) — the fork's
                                            `means2d.has_hit_any_pixels`, internal/optimizers.py:39 */,
                       void* stream);

/*    5b. Same backward with the gradients delivered as ONE packed row per splat:
 *      v_packed [N, packed_stride], packed_stride >= 6 + D (+2 when absgrad != 0); 16 makes every row one 64-B line:
 *        (dL/dx, dL/dy, dL/dconic a, b, c, dL/dopacity, dL/dcolour[0..D), [sum|dL/dx|, sum|dL/dy|]),
 *    zero-initialised by the caller.  One atomic instruction then covers contiguous components of a few
 *    splat rows instead of 64 scattered dwords. */
int gspl_composite_bwd_packed(int N, int64_t n_isects, int D, int mode, int layout,
                              const float* means2d, const float* conics, const float* colors,
                              const float* opacities, const float* backgrounds /*nullable*/,
                              int width, int height, int tile_size, int tile_w, int tile_h,
                              const int32_t* offsets, const int32_t* flatten_ids,
                              const float* final_Ts, const int32_t* last_ids,
                              const float* v_out_colors, const float* v_out_alphas /*nullable*/,
                              float* v_packed, int packed_stride /* floats per row, >= 6+D(+2) */, int absgrad,
                              uint8_t* hit_flags /*nullable*/, void* stream);

/* Deterministic (debug) mode of gspl_composite_bwd_packed (and of everything built on it: the fused Inria backward, the staged
 * rasterizers): the per-splat gradient rows are added up in list order instead of by fp32 atomics in dispatch order, so two runs give
 * the same bits.  Costs three extra passes over the list entries and stream-ordered scratch (hipMallocAsync); needs the list length
 * on the host (n_isects >= 0) and 16-pixel list tiles.  Returns the previous setting.  Process-wide.  Additive entries. */
int gspl_set_deterministic(int on);
int gspl_get_deterministic(void);
/* Name of the kernel template the two backward entry points launch in this build (profile look-ups in bench.py). */
const char* gspl_composite_bwd_kernel_name(void);

/* ------------------------------------------------------------------------------------------
 * 6. Inria-convention preprocess (the front half of the fused `GaussianRasterizer`).
 *    Replaces `diff_gaussian_rasterization.GaussianRasterizer.forward` up to the sort
 *    (vanilla_renderer.py:62-77,111-120): frustum cull (view z <= 0.2), cov3D from scale/rotation
 *    (or cov3D_precomp [N,6]), EWA cov2D + 0.3 low-pass, conic, radius, NDC->pixel mean,
 *    SH->RGB with +0.5 / clamp (or colors_precomp [N,3]).
 *      viewmatrix [16], projmatrix [16]: the reference's transposed (row-vector) 4x4s, device
 *      (internal/cameras/cameras.py:147-189); campos [3] device.
 *    Outputs: radii i32 [N], means2d [N,2] (pixels, integer-centred), depths [N], conics [N,3],
 *             colors [N,3], clamped u8 [N,3], cov3d [N,6] (saved for backward).
 *    `phases` selects the geometry kernel, the colour kernel (which reads the radii the geometry
 *    kernel wrote), or both; a caller that bins between the two hides the sort-size read-back of
 *    gspl_bin_count behind the colour kernel.
 * ---------------------------------------------------------------------------------------- */
enum { GSPL_INRIA_GEOMETRY = 1, GSPL_INRIA_COLOURS = 2, GSPL_INRIA_ALL = 3 };
int gspl_inria_preprocess_fwd(int N, int degree, int n_coeffs,
                              const float* means, const float* scales /*nullable*/,
                              const float* quats /*nullable*/, const float* cov3d_precomp /*nullable*/,
                              const float* shs /*[N,n_coeffs,3] nullable; with shs_rest: the DC rows [N,1,3]*/,
                              const float* shs_rest /*nullable [N,n_coeffs-1,3]: the reference's model keeps the coefficients as two
                                                      parameters, shs_dc and shs_rest (vanilla_gaussian.py:266-300, `get_shs` = a
                                                      torch.cat per step); given both, they are read where they are*/,
                              const float* colors_precomp /*nullable*/,
                              const float* viewmatrix, const float* projmatrix, const float* campos,
                              int width, int height, int tile_size,
                              float tanfovx, float tanfovy, float scale_modifier,
                              int32_t* radii, float* means2d, float* depths, float* conics,
                              float* colors, uint8_t* clamped, float* cov3d,
                              float* sh_jac /* nullable [N,9]: the colour kernel leaves d colour / d (unit view direction) here, and
                                               a backward that is handed it finds the view-direction part of v_means without
                                               reading the 12 n_coeffs bytes of coefficients per splat again */,
                              int phases /* GSPL_INRIA_GEOMETRY | GSPL_INRIA_COLOURS */,
                              void* stream);
/*    Backward.  v_means2d is the composite kernel's pixel-unit gradient [N,2]; the returned
 *    v_means2d_ndc [N,3] is what the reference exposes as `viewspace_points.grad`
 *    (pixel gradient x 0.5*W, 0.5*H; vanilla_renderer.py:55-56).
 *    v_shs [N,n_coeffs,3], v_cov3d_precomp [N,6], v_colors_precomp nullable as their inputs. */
int gspl_inria_preprocess_bwd(int N, int degree, int n_coeffs,
                              const float* means, const float* scales /*nullable*/,
                              const float* quats /*nullable*/, const float* cov3d /*[N,6] from fwd*/,
                              const float* shs /*nullable*/, const float* shs_rest /*nullable, as in the forward*/,
                              const float* viewmatrix, const float* projmatrix, const float* campos,
                              int width, int height,
                              float tanfovx, float tanfovy, float scale_modifier,
                              const int32_t* radii, const uint8_t* clamped,
                              const float* v_means2d, const float* v_conics, const float* v_colors,
                              int grad_stride /* 0: dense [N,2],[N,3],[N,3]; k: columns of one packed [N,k] buffer */,
                              float* v_means, float* v_scales /*nullable*/, float* v_quats /*nullable*/,
                              float* v_cov3d_precomp /*nullable*/, float* v_shs /*nullable*/,
                              float* v_shs_rest /*nullable; given iff shs_rest is: v_shs is then [N,1,3], this one [N,n_coeffs-1,3]*/,
                              float* v_colors_precomp /*nullable*/, float* v_means2d_ndc,
                              const float* v_opacities_packed /*nullable: the opacity column of the packed buffer */,
                              float* v_opacities /*nullable: [N], receives that column densely (the optimizer's
                                                   gradient is then a contiguous tensor, not a strided view) */,
                              const float* sh_jac /*nullable: from the forward*/,
                              void* stream);

/* ------------------------------------------------------------------------------------------
 * 6b. The WHOLE Inria rasterizer in one call per direction ("fused gs_rasterize_vanilla_fwd/bwd, Inria
 *    argument list"): what `diff_gaussian_rasterization`'s `_C.rasterize_gaussians` / `_C.rasterize_gaussians_backward` are to
 *    the reference's wrapper (call site internal/renderers/vanilla_renderer.py:62-120).  Preprocess (geometry, then colours on
 *    `side_stream` next to the depth sort), list-only binning with lossless tile culling and the one host read-back of the
 *    frame (waited for INSIDE the call), compositing.  Memory comes from the caller through `alloc` — the Inria library's own
 *    resize-call-back pattern: the returned device pointers must stay valid until the matching backward has run (the Python
 *    side keeps the torch byte tensors in the autograd context).  Tags tell the call-back what a block is for; one block per tag
 *    and call, except GSPL_BUF_LISTS_WORK, GSPL_BUF_LISTS and GSPL_BUF_CHECKPOINTS, which are asked for a second time when the
 *    speculative emission's guess of the list length (`capacity_hint`, e.g. the previous frame's x 1.25; 0 = no speculation)
 *    was too low: the second block replaces the first.  No hipMalloc, no global state.
 *    out_color [3,H,W], radii [N] are caller-allocated outputs; `state` receives the pointers the backward needs and
 *    n_isects (the list length — feed it back as the next frame's hint); its `flags` field is read BEFORE it is filled.
 * ---------------------------------------------------------------------------------------- */
enum { GSPL_BUF_GEOMETRY = 1, GSPL_BUF_BINNING = 2, GSPL_BUF_IMAGE = 3, GSPL_BUF_LISTS_WORK = 4, GSPL_BUF_LISTS = 5,
       GSPL_BUF_CHECKPOINTS = 6 /* segmented backward: 4 KB per 256 list entries of capacity; kept until the backward like IMAGE / LISTS */,
       GSPL_BUF_PACKED = 7 /* ABI 35, only with GSPL_INRIA_WILL_BACKWARD: 36 N bytes (rounded up to 16), the backward's per-splat rows
                              x y | a b c | opacity | r g b, CLEARED by the forward's compositing kernel — hand it to the backward as `packed` */ };
typedef void* (*gspl_alloc_fn)(void* ctx, int tag, size_t bytes);      /* device memory, 256-byte aligned; NULL = failure */
typedef struct gspl_inria_state {
    int N, width, height;
    int64_t n_isects;
    float* means2d; float* depths; float* conics; float* colors; uint8_t* clamped; float* cov3d; float* sh_jac;      /* GSPL_BUF_GEOMETRY */
    float* alphas; float* final_Ts; int32_t* last_ids; int32_t* offsets;                               /* GSPL_BUF_IMAGE */
    int32_t* flatten_ids;                                                                              /* GSPL_BUF_LISTS */
    float* opacities;      /* GSPL_BUF_GEOMETRY: the opacities compositing read — the caller's tensor, or with GSPL_INRIA_RAW_PARAMS
                              sigmoid(raw) [N] as the forward stored it */
    int flags;             /* IN (forward; the backward reads it back): 0 — a zeroed struct — or GSPL_INRIA_RAW_PARAMS | GSPL_INRIA_NO_SEGMENTS
                              | GSPL_INRIA_ANTIALIAS | GSPL_INRIA_INVDEPTH ... (below) */
    /* segmented backward (ABI 33): per-pixel checkpoints the forward left every 256 list entries and the words
     * [count | - | work items seg_slots] in front of them (one GSPL_BUF_CHECKPOINTS block); seg_ckpt == NULL: this frame is not segmented */
    void* seg_ckpt; uint32_t* seg_words; uint32_t seg_slots; uint32_t seg_reserved;
    /* densification statistics inside the backward (ABI 34; IN, read by gspl_rasterize_inria_bwd / _bwd_adam only — the forward clears
     * them, the caller sets them between the two calls): not NULL = the preprocess-backward kernel applies section 11's update to the
     * rows it has just produced the screen-space gradient of (visible = radii > 0, no scale, v_means2D_ndc as `grad`), with the same
     * arithmetic as gspl_densify_stats — the density controller's launch after the backward goes away.  accum and denom go together. */
    float* stats_accum; float* stats_denom; float* stats_max_radii;
} gspl_inria_state;
/* GSPL_INRIA_RAW_PARAMS: `scales`, `rotations`, `opacities` are the model's RAW parameters and the activations of the reference's
 *    model — scale_activation = exp, rotation_activation = F.normalize (x / max(|x|, 1e-12)), opacity_activation = sigmoid
 *    (internal/models/vanilla_gaussian.py:345-358, applied by `get_scaling` / `get_rotation` / `get_opacity` in
 *    vanilla_renderer.py:62-77 before every render, differentiated by autograd after every backward) — run inside the preprocess
 *    kernels; the backward returns the gradients of the raw parameters.  Needs scales + rotations (no cov3D_precomp). */
enum { GSPL_INRIA_RAW_PARAMS = 1,
       GSPL_INRIA_NO_SEGMENTS = 2 /* never: the backward walks every tile's list with one workgroup, however long */,
       GSPL_INRIA_FORCE_SEGMENTS = 4 /* always take checkpoints (default: only while walks longer than a segment are being met) */,
       GSPL_INRIA_WILL_BACKWARD = 8 /* ABI 35, IN: a backward will follow — the forward asks `alloc` for GSPL_BUF_PACKED and its compositing
                                       kernel (VALU-bound, the memory system idle) clears it, instead of a 7 us fill command in front of the
                                       backward's first kernel */,
       GSPL_INRIA_PACKED_READY = 16 /* OUT (set by the forward in state->flags): the GSPL_BUF_PACKED block is cleared and the backward will NOT
                                       clear its `packed` argument — which must be that block */,
       GSPL_INRIA_ANTIALIAS = 32 /* ABI 36, IN: the Mip-Splatting 2D filter (graphdeco `dr_aa` / Taming 3DGS `antialiasing=True`): the
                                    opacity compositing and the binning read is opacity * comp, comp = sqrt(max(2.5e-5, det0 / det1)) with
                                    det0 / det1 the determinant of the 2D covariance before / after its +0.3 dilation; state->opacities
                                    then always holds those effective opacities [N] (activated first with GSPL_INRIA_RAW_PARAMS) and the
                                    backward chains the compensation into the covariance.  Radii and conics are unchanged */,
       GSPL_INRIA_INVDEPTH = 128 /* ABI 36, IN: a 4th composited channel, 1 / z of the view-space depth (background 0): out_color is
                                   [4,H,W] (colour | inverse depth), `bg` holds FOUR values (the caller's 3 and a 0), state->colors is
                                   [N,4], GSPL_BUF_PACKED is 40 N bytes (rounded up to 16) and the backward's `packed` [N,10]
                                   (x y | a b c | opacity | r g b | 1/z) and v_out_color [4,H,W].  The segmented backward carries the
                                   4th channel: GSPL_BUF_CHECKPOINTS grows by one float per checkpoint (5 KB per 256 list entries of
                                   capacity), and GSPL_INRIA_FORCE_SEGMENTS / NO_SEGMENTS mean what they mean without it.  Neither this
                                   bit nor GSPL_INRIA_ANTIALIAS is accepted by gspl_rasterize_inria_bwd_adam.  (Bit 64 stays unused:
                                   callers have used it as the example of an unknown bit the forward refuses.) */ };
size_t gspl_rasterize_inria_geometry_bytes(int N);      /* the GSPL_BUF_GEOMETRY request of a frame WITHOUT GSPL_INRIA_INVDEPTH; with it the
                                                          request is larger (16 N more bytes, rounded up to 256: the [N,4] rows) */
size_t gspl_rasterize_inria_image_bytes(int width, int height);
size_t gspl_inria_state_bytes(void);      /* sizeof(gspl_inria_state) as the library was built: a binding checks its own layout against it */
int gspl_rasterize_inria_fwd(int N, int degree, int n_coeffs,
                             const float* means3D, const float* scales /*nullable*/, const float* rotations /*nullable*/,
                             const float* cov3D_precomp /*nullable*/, const float* shs /*nullable*/,
                             const float* shs_rest /*nullable: see gspl_inria_preprocess_fwd*/, const float* colors_precomp /*nullable*/,
                             const float* opacities,
                             const float* viewmatrix, const float* projmatrix, const float* campos, const float* bg,
                             int width, int height, float tanfovx, float tanfovy, float scale_modifier,
                             gspl_alloc_fn alloc, void* alloc_ctx, int64_t capacity_hint,
                             float* out_color, int32_t* radii, gspl_inria_state* state,
                             void* stream, void* side_stream /*nullable: colours on `stream`*/);
/*    Backward: packed [N,9] f32 scratch and hit_flags [N] u8 (nullable) are cleared inside; every v_* is caller-allocated
 *    ([N,3], [N,3] NDC-scaled, [N,n_coeffs,3] (or [N,1,3] and [N,n_coeffs-1,3] with shs_rest) | [N,3], [N], [N,3], [N,4] | [N,6]; the ones that do not apply are NULL). */
int gspl_rasterize_inria_bwd(int degree, int n_coeffs,
                             const float* means3D, const float* scales, const float* rotations, const float* shs, const float* shs_rest,
                             const float* opacities,
                             const float* viewmatrix, const float* projmatrix, const float* campos, const float* bg,
                             float tanfovx, float tanfovy, float scale_modifier,
                             const int32_t* radii, const gspl_inria_state* state, const float* v_out_color,
                             float* packed, uint8_t* hit_flags /*nullable*/,
                             float* v_means3D, float* v_means2D_ndc, float* v_shs, float* v_shs_rest, float* v_colors_precomp, float* v_opacities,
                             float* v_scales, float* v_rotations, float* v_cov3D, void* stream);
/* The same backward for frames in which most splats get no gradient (additive entry, GSPL_ABI_VERSION stays 39; a saturated scene
 * blends ~50 splats per pixel and leaves nine rows in ten exactly zero).  The v_* arrays are cleared on the library's low-priority stream
 * BESIDE the compositing backward (forked from and joined into `stream` with events), and the per-splat kernels behind it then read
 * the geometry of, and write, only the rows whose packed gradient row is not all zero; the densification statistics of the state are
 * applied to every visible row as always.  grad_rows [N] u8 (written): 1 = the row may hold a non-zero gradient, 0 = all 59 floats
 * (and v_means2D_ndc) of the row are zero.  Every output equals gspl_rasterize_inria_bwd's as a value; where that one computes a zero
 * from a negative factor it writes -0, this one leaves +0. */
int gspl_rasterize_inria_bwd_sparse(int degree, int n_coeffs,
                                    const float* means3D, const float* scales, const float* rotations, const float* shs, const float* shs_rest,
                                    const float* opacities,
                                    const float* viewmatrix, const float* projmatrix, const float* campos, const float* bg,
                                    float tanfovx, float tanfovy, float scale_modifier,
                                    const int32_t* radii, const gspl_inria_state* state, const float* v_out_color,
                                    float* packed, uint8_t* hit_flags /*nullable*/,
                                    float* v_means3D, float* v_means2D_ndc, float* v_shs, float* v_shs_rest, float* v_colors_precomp, float* v_opacities,
                                    float* v_scales, float* v_rotations, float* v_cov3D, uint8_t* grad_rows, void* stream);

/* The backward with the OPTIMIZER INSIDE (additive entry, round 5): the per-Gaussian kernels that end the backward apply the Adam update
 * to the rows they have just produced the gradient of — moments read and written once, parameters written once, NO parameter gradient in
 * HBM (236 B per Gaussian written by the backward and read back by the optimizer launch otherwise: the two-kernel form of
 * internal/optimizers.py:14-22 / internal/models/vanilla_gaussian.py:266-300 behind gaussian_splatting.py:380-397).
 * means3D ... opacities are the PARAMETERS, updated in place (raw parameters with GSPL_INRIA_RAW_PARAMS in the state's flags, else
 * the activated tensors the forward was given); every row is updated, a Gaussian the frame does not see with a zero gradient
 * (torch.optim.Adam semantics).  shs_rest == NULL: `shs` holds all n_coeffs rows and plan->shs its moments.  scratch_means [N,3] f32
 * and packed [N,9] are scratch; v_means2D_ndc [N,3] (the screen-space gradient) is the one gradient written.
 * Same arithmetic as gspl_rasterize_inria_bwd followed by gspl_selective_adam with no mask (bit-identical parameters and moments for
 * identical gradients: tests/test_fused_backward_adam.py). */
typedef struct gspl_bwd_adam_tensor {
    float* exp_avg;              /* first / second moment, shape of the parameter, f32 contiguous */
    float* exp_avg_sq;
    float lr, beta1, beta2, eps;
    float bias_correction1;      /* 1 - beta1^t   (1: gsplat's uncorrected update) */
    float bias_correction2_sqrt; /* sqrt(1 - beta2^t)   (1: uncorrected) */
} gspl_bwd_adam_tensor;
typedef struct gspl_bwd_adam_plan {
    gspl_bwd_adam_tensor means, scales, rotations, opacities, shs, shs_rest;
} gspl_bwd_adam_plan;
int gspl_rasterize_inria_bwd_adam(int degree, int n_coeffs,
                                  float* means3D, float* scales, float* rotations, float* shs, float* shs_rest /*nullable*/, float* opacities,
                                  const float* viewmatrix, const float* projmatrix, const float* campos, const float* bg,
                                  float tanfovx, float tanfovy, float scale_modifier,
                                  const int32_t* radii, const gspl_inria_state* state, const float* v_out_color,
                                  float* packed, uint8_t* hit_flags /*nullable*/, float* scratch_means, float* v_means2D_ndc,
                                  const gspl_bwd_adam_plan* plan /* host */, void* stream);

/* ------------------------------------------------------------------------------------------
 * 6c. The 2D Gaussian Splatting (surfel) rasterizer in one call per direction (ABI 37): what `diff_surfel_rasterization`'s
 *    native calls are to the reference's `Vanilla2DGSRenderer` (internal/renderers/vanilla_2dgs_renderer.py:50-90).  The rule is the
 *    published 2DGS rasterizer restated in this library's Inria conventions (csrc/surfel.hip; parity with the CUDA package is
 *    unpinned, an fp64 oracle pins the restatement): each splat is a disc in the plane of its two scaled tangent axes, each pixel
 *    intersects its ray with that plane.  Memory comes from `alloc` as in 6b (tags GEOMETRY, IMAGE, BINNING, LISTS_WORK, LISTS; the
 *    deterministic backward asks for GSPL_BUF_SURFEL_ENTRIES); no hipMalloc, one host read-back of the list length per frame.
 *      scales [N,2] (the two tangent scales), rotations [N,4] (w,x,y,z; normalised inside), opacities [N]; shs [N,n_coeffs,3] with
 *      campos, or colors_precomp [N,3]; bg [3].  No precomputed transform (the reference passes cov3D_precomp = None).
 *    Outputs: out_color [3,H,W] (+ T bg), out_allmap [7,H,W] = depth | alpha | view-space normal (3) | median depth | distortion
 *             (no background), radii i32 [N] (0 = culled).  `state` receives what the backward needs.
 *    Backward: the exact derivative with the 0.99 alpha clamp straight-through and no gradient through a clamped SH channel, except
 *    v_means2D [N,3]: upstream's densification proxy (dL/dTu.z Tw.z W/2, dL/dTv.z Tw.z H/2, 0) from the compositing backward's
 *    gradient of the splat's transform alone.  v_rows [N,18] f32 is scratch (cleared inside); exactly one of v_shs [N,n_coeffs,3] /
 *    v_colors_precomp [N,3]; v_scales [N,2], v_rotations [N,4], v_opacities [N], v_means3D [N,3].  gspl_get_deterministic(): the
 *    per-splat gradients are added up in list order (bit-reproducible).
 * ---------------------------------------------------------------------------------------- */
enum { GSPL_BUF_SURFEL_ENTRIES = 8 /* deterministic surfel backward: 72 B per list entry + the id sort's keys and workspace */ };
typedef struct gspl_surfel_state {
    int N, width, height;
    int64_t n_isects;
    float* rec;            /* [N,16] Tu Tv Tw | centre | opacity | view normal | 0   (GSPL_BUF_GEOMETRY, as the next four) */
    float* means2d; float* depths; float* colors; uint8_t* clamped;
    float* final_T; float* M1; float* M2; int32_t* last_contrib; int32_t* median_contrib; int32_t* offsets;      /* GSPL_BUF_IMAGE */
    int32_t* flatten_ids;                                                                                         /* GSPL_BUF_LISTS */
} gspl_surfel_state;
size_t gspl_surfel_state_bytes(void);      /* sizeof(gspl_surfel_state) as the library was built */
int gspl_rasterize_surfel_fwd(int N, int degree, int n_coeffs,
                              const float* means3D, const float* scales, const float* rotations,
                              const float* shs /*nullable*/, const float* colors_precomp /*nullable*/, const float* opacities,
                              const float* viewmatrix, const float* projmatrix, const float* campos, const float* bg,
                              int width, int height, float scale_modifier,
                              gspl_alloc_fn alloc, void* alloc_ctx,
                              float* out_color, float* out_allmap, int32_t* radii, gspl_surfel_state* state, void* stream);
int gspl_rasterize_surfel_bwd(int degree, int n_coeffs,
                              const float* means3D, const float* scales, const float* rotations, const float* shs /*nullable*/,
                              const float* viewmatrix, const float* projmatrix, const float* campos, const float* bg, float scale_modifier,
                              const int32_t* radii, const gspl_surfel_state* state, const float* v_out_color, const float* v_out_allmap,
                              gspl_alloc_fn alloc /*nullable outside the deterministic mode*/, void* alloc_ctx, float* v_rows,
                              float* v_means3D, float* v_means2D, float* v_shs /*nullable*/, float* v_colors_precomp /*nullable*/,
                              float* v_opacities, float* v_scales, float* v_rotations, void* stream);

/* A per-device stream of the LOWEST priority the device offers, created on first use and kept: a `side_stream` for
 * gspl_rasterize_inria_fwd whose colour kernel then yields to the kernels on the caller's stream.  NULL on failure. */
void* gspl_low_priority_stream(void);

/* Timing of the compositing launches inside the fused calls (bench.py: the roofline of the graded kernel needs its launch
 * duration from HIP events on the launch stream, and the launches are no longer visible from the host language).
 * gspl_profile_enable(k) starts recording every k-th launch (k = 1: all; an event pair costs the stream ~6 us of idle time on
 * either side of the launch) and drops what was recorded, gspl_profile_read synchronises and returns the count and the summed
 * duration of the timed forward (which = 0) or backward (1) compositing launches since then; enable(0) stops. */
int gspl_profile_enable(int period);
int gspl_profile_enable2(int period_fwd, int period_bwd);      /* the two directions apart (0 = that direction is not timed) */
int gspl_profile_read(int which, int* count, float* total_ms);

/* ------------------------------------------------------------------------------------------
 * 6c. Visible-splat records of the Gaussian-sharded multi-GPU renderer: pack / unpack, forward and backward.
 *    Replaces the per-camera `torch.concat` + boolean-mask selection before, and the `torch.split` after, the all-to-all of
 *    internal/renderers/gsplat_distributed_renderer.py:313-414.  Record = 12 fp32 (48 B):
 *        [x, y, depth, conic a, b, c, compensation, opacity, r, g, b, radius (int32 bits)]
 *    pack: every (camera, local splat) with radius > 0 -> one record, grouped by camera (= destination rank), splat order kept.
 *      records: room for C*N rows; slots [C,N] i32 = row of the pair's record or -1 (the backward's route); ends [C] i64 =
 *      one past each camera's last row (device), host_ends (nullable) the same in pinned host memory, stored by the kernel.
 *    pack_bwd: writes EVERY row of every gradient tensor (zeros where invisible); v_opacities [N] summed over the cameras.
 *    unpack: received records -> per-quantity tensors; fold_compensation: opacities = opacity x compensation (anti-aliased
 *      mode), with the product rule applied by unpack_bwd.  Strides (floats per row, 0 = dense) let unpack_bwd read the columns
 *      of gspl_composite_bwd_packed's row buffer in place.
 * ---------------------------------------------------------------------------------------- */
#define GSPL_RECORD_FLOATS 12
size_t gspl_records_workspace_bytes(int C, int N);
int gspl_records_pack_fwd(int C, int N, const int32_t* radii, const float* means2d, const float* depths, const float* conics,
                          const float* compensations /*nullable = 1*/, const float* opacities /*[N]*/, const float* colors /*[C,N,3]*/,
                          float* records, int32_t* slots, int64_t* ends, int64_t* host_ends /*nullable*/,
                          void* workspace, size_t workspace_bytes, void* stream);
/* The pack in two phases (same slots, ends and records): COUNT needs the radii only — the per-camera ends are on their way to the
 * host (`host_ends`, pinned) before the colours of the frame exist, so the exchange of the counts (gsplat_distributed_renderer.py:
 * 141-160) overlaps the colour kernel —, SCATTER writes the records to their slots.  Workspace as gspl_records_pack_fwd (COUNT only).
 * Additive entries (no existing signature changed: the ABI version stays). */
int gspl_records_count_fwd(int C, int N, const int32_t* radii, int32_t* slots, int64_t* ends, int64_t* host_ends /*nullable*/,
                           void* workspace, size_t workspace_bytes, void* stream);
int gspl_records_scatter_fwd(int C, int N, const int32_t* radii, const int32_t* slots, const float* means2d, const float* depths,
                             const float* conics, const float* compensations /*nullable = 1*/, const float* opacities /*[N]*/,
                             const float* colors /*[C,N,3]*/, float* records, void* stream);
/* The fixed-size exchange format: one record per (camera, local splat), camera-major, rows of invisible splats zeroed (radius 0
 * keeps them out of the receiver's lists); slots[i] = i for the visible rows, -1 otherwise (input of gspl_records_pack_bwd).  No
 * count, no workspace, nothing the host has to wait for: every size of the exchange is known before the step starts. */
int gspl_records_pad_fwd(int C, int N, const int32_t* radii, const float* means2d, const float* depths, const float* conics,
                         const float* compensations /*nullable = 1*/, const float* opacities /*[N]*/, const float* colors /*[C,N,3]*/,
                         float* records /*[C*N,12]*/, int32_t* slots /*[C,N]*/, void* stream);
int gspl_records_pack_bwd(int C, int N, const int32_t* slots, const float* v_records,
                          float* v_means2d, float* v_depths, float* v_conics, float* v_compensations /*nullable*/, float* v_opacities,
                          float* v_colors, void* stream);
int gspl_records_unpack_fwd(int64_t M, int fold_compensation, const float* records, int32_t* radii, float* means2d, float* depths,
                            float* conics, float* opacities, float* colors, void* stream);
int gspl_records_unpack_bwd(int64_t M, int fold_compensation, const float* records,
                            const float* v_means2d /*nullable = 0*/, int v_means2d_stride, const float* v_depths /*nullable*/,
                            const float* v_conics /*nullable*/, int v_conics_stride, const float* v_opacities /*nullable*/, int v_opacities_stride,
                            const float* v_colors /*nullable*/, int v_colors_stride, float* v_records, void* stream);

/*    Direct peer-to-peer transport of the records (csrc/peer.hip): instead of an all-to-all collective, every rank writes its rows
 *    straight into the receive buffer of the destination rank — device memory of the peer process mapped through HIP IPC, reached
 *    over xGMI (or the same GPU) — and raises one flag word per destination; the receiver's stream waits for its flag words.
 *    Replaces torch.distributed.nn.functional.all_to_all of gsplat_distributed_renderer.py:141-202 in the per-step exchange.
 *      gspl_peer_alloc   fine-grained device memory (remote stores are visible without an L2 invalidation) + its 64-byte IPC handle,
 *                        which the host sends to the peers once (e.g. torch.distributed.all_gather_object at training_setup)
 *      gspl_peer_open    maps a peer's buffer from its handle (gspl_peer_close unmaps; gspl_peer_free releases an own buffer)
 *      gspl_peer_put_rows  one launch: rows [row_begin[d], row_begin[d+1]) of `rows` -> dst[d] (16-byte stores; up to 16 destinations)
 *      gspl_peer_signal  one launch behind it: system-scope release fence, then `value` into every flag word
 *      gspl_peer_wait    one launch on the receiver: polls its n_src flag words until all are >= value; gives up after max_polls
 *                        polls and stores 1 + source into *error (a lost peer must not hang the GPU; the host checks the word)
 *    Additive entries (no existing signature changed: the ABI version stays). */
int gspl_peer_alloc(size_t bytes, void** ptr, void* handle_out /* 64 bytes */);
int gspl_peer_open(const void* handle /* 64 bytes */, void** ptr);
int gspl_peer_close(void* ptr);
int gspl_peer_free(void* ptr);
int gspl_peer_put_rows(int n_dst, const float* rows, const int64_t* row_begin /* host, [n_dst + 1] */,
                       void* const* dst /* host, [n_dst] device pointers */, int floats_per_row /* multiple of 4 */, void* stream);
int gspl_peer_signal(int n_dst, void* const* flags /* host, [n_dst] device pointers to 8-byte words */, uint64_t value, void* stream);
int gspl_peer_wait(const uint64_t* flags /* device, [n_src] */, int n_src, uint64_t value, uint64_t max_polls,
                   int32_t* error /* device-visible word: device memory, or PINNED HOST memory the host can read without synchronising */, void* stream);

/* ------------------------------------------------------------------------------------------
 * 7. Mean squared distance to the 3 nearest neighbours ("next" row SURVEY.md §8f rank 1).
 *    Replaces `simple_knn._C.distCUDA2` at its one call site, the initial scales of
 *    `VanillaGaussianModel.setup_from_pcd` (internal/models/vanilla_gaussian.py:122-125):
 *        out[i] = mean over the 3 nearest OTHER points j of |p_i - p_j|^2     (fp32)
 *    points [N,3] f32, out [N] f32.  Exact (uniform grid + expanding shells).  With fewer than three
 *    other points the mean is taken over those that exist (0 for a single point).
 * ---------------------------------------------------------------------------------------- */
size_t gspl_knn_workspace_bytes(int N);
int gspl_knn3_mean_dist2(int N, const float* points, float* out,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * 8. Fused photometric loss terms ("next" row SURVEY.md §8f rank 2): mean |x - y| and mean SSIM.
 *    Replaces `l1_loss` + `ssim` (internal/utils/ssim.py:17-63) and the opt-in `fused_ssim` package
 *    (internal/metrics/vanilla_metrics.py:35-39) in  loss = (1-l) L1 + l (1 - SSIM)  (:57-70).
 *    SSIM: 11x11 Gaussian window (sigma 1.5, separable), zero padding, C1 = 0.01^2, C2 = 0.03^2, mean
 *    over all planes * H * W elements.  img1, img2: [planes, H, W] f32 contiguous (planes = batch * channels).
 *      fwd: out_means[2] = (mean |img1-img2|, mean SSIM); dm_* [planes,H,W] (all three or none): the
 *           derivative maps the backward needs (pass NULL for evaluation only).
 *      bwd: v_img1 = weight_l1 * v_l1_mean * d(L1)/d(img1) + weight_ssim * v_ssim_mean * d(SSIM)/d(img1);
 *           v_*_mean are device scalars (NULL = 1); dm_* NULL drops the SSIM term.
 * ---------------------------------------------------------------------------------------- */
size_t gspl_loss_workspace_bytes(int planes, int H, int W);
int gspl_loss_l1_ssim_fwd(int planes, int H, int W, const float* img1, const float* img2,
                          float* out_means, float* dm_dmu1 /*nullable*/, float* dm_ds1, float* dm_ds12,
                          void* workspace, size_t workspace_bytes, void* stream);
/*    The training loss in one go: out_terms[3] = (mean|x-y|, mean SSIM, weight_l1 * L1 + weight_ssim * (1 - SSIM)),
 *    i.e. vanilla_metrics.py:66-68 with weight_l1 = 1 - lambda_dssim, weight_ssim = lambda_dssim.  Its backward is
 *    gspl_loss_l1_ssim_bwd with both upstream pointers = dL/dloss and weights (weight_l1, -weight_ssim). */
int gspl_loss_photometric_fwd(int planes, int H, int W, const float* img1, const float* img2,
                              float weight_l1, float weight_ssim, float* out_terms,
                              float* dm_dmu1 /*nullable*/, float* dm_ds1, float* dm_ds12,
                              void* workspace, size_t workspace_bytes, void* stream);
int gspl_loss_l1_ssim_bwd(int planes, int H, int W, const float* img1, const float* img2,
                          const float* dm_dmu1 /*nullable*/, const float* dm_ds1, const float* dm_ds12,
                          const float* v_l1_mean /*nullable*/, const float* v_ssim_mean /*nullable*/,
                          float weight_l1, float weight_ssim, float* v_img1, void* stream);

/* ------------------------------------------------------------------------------------------
 * 9. Visibility-masked fused Adam over all per-Gaussian tensors ("next" row SURVEY.md §8f rank 3).
 *    Replaces gsplat `SelectiveAdam` (internal/optimizers.py:26-58) and, with visible = NULL and the
 *    bias corrections of step t, the per-property `torch.optim.Adam` steps (vanilla_gaussian.py:266-300).
 *    For every element of every row n with visible[n] != 0 (NULL: all rows):
 *        m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
 *        p -= (lr / bias_correction1) * m / (sqrt(v) / bias_correction2_sqrt + eps)
 *    (bias_correction1 = 1 - b1^t, bias_correction2_sqrt = sqrt(1 - b2^t); pass 1, 1 for gsplat's
 *    uncorrected update).  Masked rows keep parameter and moments.  All tensors are [N, row_elems]
 *    f32, contiguous, 16-byte aligned; up to GSPL_ADAM_MAX_TENSORS per call, one launch.
 * ---------------------------------------------------------------------------------------- */
enum { GSPL_ADAM_MAX_TENSORS = 16 };
typedef struct gspl_adam_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    float lr;
    int32_t row_elems;
} gspl_adam_tensor;
int gspl_selective_adam(int n_tensors, const gspl_adam_tensor* tensors /* host array */, int N,
                        const uint8_t* visible /*nullable, device [N]*/,
                        float beta1, float beta2, float eps, float bias_correction1, float bias_correction2_sqrt,
                        void* stream);
/* The same update with at most `max_blocks` workgroups per tensor (0 = no limit): for a launch that shares the device with the
 * kernels of another stream (optimizers.FusedAdam(deferred=...): the shs_rest update next to the following frame's binning). */
int gspl_selective_adam_limited(int n_tensors, const gspl_adam_tensor* tensors, int N, const uint8_t* visible /*nullable*/,
                                float beta1, float beta2, float eps, float bias_correction1, float bias_correction2_sqrt,
                                int max_blocks, void* stream);
/* The same update told which rows have a gradient at all (additive entry, GSPL_ABI_VERSION stays 39): grad_rows [N] u8, device,
 * nullable; 0 = EVERY gradient element of that row, in every tensor of the call, is zero (gspl_rasterize_inria_bwd_sparse leaves such an
 * array).  All rows are updated as always (Adam moves a row with g = 0); in tensors of 32 or more floats per row a 16-byte chunk whose
 * rows all carry 0 is updated with a zero from a register instead of its gradient from memory.  Same parameters and moments. */
int gspl_selective_adam_rows(int n_tensors, const gspl_adam_tensor* tensors, int N, const uint8_t* visible /*nullable*/,
                             const uint8_t* grad_rows /*nullable*/,
                             float beta1, float beta2, float eps, float bias_correction1, float bias_correction2_sqrt,
                             int max_blocks, void* stream);

/* ------------------------------------------------------------------------------------------
 * 10. Stable LSD radix sort of the binning stage, exported for the parity tests.
 *    The depth sort inside gspl_bin_count (depth keys + splat ids, u32 pairs, first pass counted by the key pass
 *    itself) runs on this sort (csrc/sort.hip: count -> scatter per pass, no inter-workgroup waiting); the u64 keys-only entry
 *    point is the same kernels at the record width of the tile sort (gspl_bin_sort runs them with a last pass that writes
 *    ids + per-tile counts).  Both stand in for the
 *    cub::DeviceRadixSort::SortPairs calls of the reference's native rasterizers (gsplat `isect_tiles`
 *    behind gsplat_v1_renderer.py:524-556, the Inria rasterizer behind vanilla_renderer.py:111): stable,
 *    ascending on key bits [begin_bit, end_bit); at most 32 selected bits (4 passes of <= 8 bits), at most
 *    2^30-1 items.  Buffer 0 holds the input and is overwritten; buffer 1 is scratch of the same size; the
 *    sorted sequence ends in buffer *result_buffer (0 or 1).
 * ---------------------------------------------------------------------------------------- */
size_t gspl_radix_sort_workspace_bytes(int64_t n, int key_bytes /* 4 or 8 */, int begin_bit, int end_bit);
int gspl_radix_sort_pairs_u32(int64_t n, uint32_t* keys0, uint32_t* keys1, uint32_t* vals0, uint32_t* vals1,
                              int begin_bit, int end_bit, int* result_buffer /* host */,
                              void* workspace, size_t workspace_bytes, void* stream);
int gspl_radix_sort_keys_u64(int64_t n, uint64_t* keys0, uint64_t* keys1, int begin_bit, int end_bit,
                             int* result_buffer /* host */, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * 11. Densification statistics of the density controller, one launch.
 *    Replaces the PyTorch lines of `VanillaDensityControllerImpl.update_states` /
 *    `_add_densification_stats` (internal/density_controllers/vanilla_density_controller.py:101-123).
 *    For every Gaussian n with visible[n] != 0 (visible == NULL: radii[n] > 0):
 *        max_radii[n] = max(max_radii[n], radii[n])                     (skipped when max_radii == NULL)
 *        accum[n]    += | (grad[n,0] * scale_x, grad[n,1] * scale_y) |_2
 *        denom[n]    += 1
 *    grad [N, grad_stride] f32 (the first two columns are read: `viewspace_points.grad` or `.absgrad`);
 *    scale: scale_dev (device float[2], e.g. the renderers' `viewspace_points_grad_scale`) when not NULL,
 *    else the two host floats (1, 1 for "no scale"); radii as int32 or float32 (one of them, or neither
 *    when a mask is given and max_radii is NULL); accum, denom, max_radii [N] f32, updated in place.
 * ---------------------------------------------------------------------------------------- */
int gspl_densify_stats(int N, const float* grad, int grad_stride, float scale_x, float scale_y,
                       const float* scale_dev /*nullable*/, const uint8_t* visible /*nullable*/,
                       const int32_t* radii_i32 /*nullable*/, const float* radii_f32 /*nullable*/,
                       float* accum, float* denom, float* max_radii /*nullable*/, void* stream);
/* The same update for the n_views (<= GSPL_STATS_MAX_VIEWS) cameras of ONE Gaussian-sharded step in one launch — the loop over
 * `projection_results_list` of `DistributedVanillaDensityControllerImpl.update_states`
 * (internal/density_controllers/distributed_vanilla_density_controller.py:22-47): grads / visible / radii_i32 are HOST arrays of
 * n_views device pointers ([N, grad_stride] f32, [N] u8 or NULL entries, [N] i32 or NULL entries; `visible` / `radii_i32` themselves may
 * be NULL); the views are applied in array order per Gaussian: the buffers equal those of n_views sequential gspl_densify_stats
 * calls bit for bit.  (ABI 35: round 6.) */
#define GSPL_STATS_MAX_VIEWS 16
int gspl_densify_stats_views(int N, int n_views, const float* const* grads, int grad_stride, float scale_x, float scale_y,
                             const float* scale_dev /*nullable*/, const uint8_t* const* visible /*nullable*/,
                             const int32_t* const* radii_i32 /*nullable*/,
                             float* accum, float* denom, float* max_radii /*nullable*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * 12. Per-splat statistics of a compositing pass (hit-pixel count / rasterize_to_weights).
 *    What LightGaussian pruning (internal/utils/light_gaussian.py:37-50 through
 *    internal/renderers/gsplat_hit_pixel_count_renderer.py:34-44 -> gsplat fork `hit_pixel_count`) and the
 *    Taming-3DGS / GNS scores (internal/density_controllers/taming_3dgs_density_controller.py:429-439 ->
 *    gsplat fork `rasterize_to_weights`) read.  Both kernels are un-vendored; the sums are restated from the
 *    published methods (PARITY UNPINNED).  Traversal and discrete rules of gspl_composite_fwd; for every splat g,
 *    over the pixels p it contributes to (alpha >= 1/255, before the pixel saturates), ADDED to the arrays:
 *        count[g] += 1;  opacity_sum[g] += opacities[g];  alpha_sum[g] += alpha;  visibility_sum[g] += alpha T;
 *        weighted_sum[g] += pixel_weights[p] alpha T;  dist_sum[g] += |p - means2d[g]|
 *    Any output may be NULL; pixel_weights [H,W] f32 is needed for weighted_sum only.  Outputs [N], zeroed by
 *    the caller (several cameras accumulate into the same arrays).
 * ---------------------------------------------------------------------------------------- */
int gspl_composite_scores(int N, int64_t n_isects, int mode,
                          const float* means2d, const float* conics, const float* opacities,
                          int width, int height, int tile_size, int tile_w, int tile_h,
                          const int32_t* offsets, const int32_t* flatten_ids, const float* pixel_weights /*nullable*/,
                          int32_t* count, float* opacity_sum, float* alpha_sum, float* visibility_sum,
                          float* weighted_sum, float* dist_sum, void* stream);

/* ------------------------------------------------------------------------------------------
 * 13. The 3DGS-MCMC density controller's per-step math (ABI 38; csrc/mcmc.hip): what `gsplat.relocation.compute_relocation`
 *    and the PyTorch lines of `MCMCDensityControllerImpl._add_xyz_noise` (internal/density_controllers/
 *    mcmc_density_controller.py:93-119) and `MCMCMetricsModuleMixin.reg_loss` (internal/metrics/mcmc_metrics.py) compute.
 *
 *  gspl_mcmc_relocation: per row m, n = clamp(ratios[m], 1, n_max), o = opacities[m] (activated), Eq. 9 of Kheradmand et al.:
 *        x = 1 - (1 - o)^(1/n)     (evaluated as -expm1(log1p(-o) / n); n = 1 gives x = o exactly)
 *        denom = sum_{i=1..n} sum_{k=0..i-1} binoms[i-1, k] (-1)^k / sqrt(k+1) x^(k+1)      (fp32, in this order)
 *        new_opacities[m] = x;  new_scales[m,:] = (o / denom) scales[m,:]
 *      opacities [M], scales [M,3] (activated), ratios i32 [M] (read only: clamped in registers), binoms [n_max, n_max]
 *      (binoms[n,k] = C(n,k)), 1 <= n_max <= 64.
 *  gspl_mcmc_perturb_means: means [N,3] IN PLACE, means += c(o) Sigma eps, with
 *        Sigma = R(q) diag(s^2) R(q)^T,  c(o) = coeff / (1 + exp(-100 ((1 - o) - 0.995))),  coeff = noise_lr * means' lr
 *      raw != 0: scales / rotations / opacities are the model's raw parameters (exp, q / max(|q|, 1e-12), sigmoid inside);
 *      raw == 0: activated values, rotations used as given.  opacities [N] (or [N,1]).  eps [N,3] from `noise` when not NULL,
 *      else eps = gspl_mcmc_randn's normals for (seed, offset), generated in registers.
 *  gspl_mcmc_randn: the generator of the noise, exported for the tests.  Gaussian i draws ONE Philox4x32-10 block with
 *        key = (lo32(seed), hi32(seed)), counter = (lo32(offset / 4), hi32(offset / 4), lo32(i), hi32(i))
 *      — curand_init(seed, subsequence = i, offset)'s first block, the layout torch's kernels use with the same generator; the
 *      caller reserves generator offsets [offset, offset + 4), offset a multiple of 4 (else GSPL_ERR_INVALID_ARG) — giving u32 words b0..b3; u_j = ((b_j >> 8) + 1) 2^-24 in (0, 1]; Box-Muller:
 *        eps0 = r01 cos(2 pi u1), eps1 = r01 sin(2 pi u1), eps2 = r23 cos(2 pi u3),   r01 = sqrt(-2 log u0), r23 = sqrt(-2 log u2)
 *      bits u32 [N,4] (nullable), normals [N,3].
 *  gspl_mcmc_reg_fwd: out[0] = opacity_w mean_i |f(o_i)|, out[1] = scale_w mean_ij |g(s_ij)| (f = sigmoid, g = exp when raw; the
 *      identity otherwise).  Deterministic: a fixed grid of gspl_mcmc_reg_partials(N) workgroups writes 2 partial sums each to
 *      `partials`, one workgroup adds them in a fixed order (no atomics).  opacities [N], scales [N,3].
 *  gspl_mcmc_reg_bwd: v_opacities [N] = grad_out[0] opacity_w / N f'(o) sign(f(o)), v_scales [N,3] = grad_out[1] scale_w / (3N)
 *      g'(s) sign(g(s)); grad_out [2] f32 on the device (the upstream gradients of out[0], out[1]).
 * ---------------------------------------------------------------------------------------- */
int gspl_mcmc_relocation(int M, int n_max, const float* opacities, const float* scales, const int32_t* ratios, const float* binoms,
                         float* new_opacities, float* new_scales, void* stream);
int gspl_mcmc_perturb_means(int N, int raw, float* means, const float* scales, const float* rotations, const float* opacities,
                            const float* noise /*nullable*/, float coeff, uint64_t seed, uint64_t offset, void* stream);
int gspl_mcmc_randn(int N, uint64_t seed, uint64_t offset, uint32_t* bits /*nullable*/, float* normals, void* stream);
int gspl_mcmc_reg_partials(int N);         /* workgroups of gspl_mcmc_reg_fwd's first pass: `partials` holds 2x as many floats */
int gspl_mcmc_reg_fwd(int N, int raw, const float* opacities, const float* scales, float opacity_w, float scale_w,
                      float* partials, float* out, void* stream);
int gspl_mcmc_reg_bwd(int N, int raw, const float* opacities, const float* scales, float opacity_w, float scale_w,
                      const float* grad_out, float* v_opacities, float* v_scales, void* stream);

/* ------------------------------------------------------------------------------------------
 * 14. Bilateral-grid slicing and its total-variation loss (ABI 39; csrc/bilagrid.hip): what `fused_bilagrid`'s `slice` and
 *    `total_variation_loss` compute for the reference's output processor (internal/output_processors/bilagrid.py), with the
 *    semantics of internal/utils/lib_bilagrid.py (`F.grid_sample(align_corners=True, padding_mode='border')`, then the affine).
 *
 *  grids [N, 12, L, GH, GW] (the 12 channels a row-major 3x4 matrix); bounds: 1 <= N <= 65535, L <= 28, GH, GW <= 1024,
 *  L GH GW <= 16384 (else GSPL_ERR_INVALID_ARG).  Images: B of H x W pixels; xy [B, H, W, 2] (xy_bstride = H W 2) or one [H, W, 2]
 *  for all (xy_bstride = 0); rgb, out, grad_out, grad_rgb hold 3 H W floats per image (image stride 3 H W), each in `layout`
 *  GSPL_LAYOUT_HWC (interleaved) or GSPL_LAYOUT_CHW (planar).  Image b uses grid idx[b * idx_stride] (i32, read on the device;
 *  idx_stride = 0: one index for all).  An index outside [0, N) reads nothing: that image's out and grad_rgb are NaN and its
 *  pixels add nothing to grad_grids.
 *  gspl_bilagrid_slice_fwd, per pixel with colour c and (x, y):
 *        z = 2 (0.299 c0 + 0.587 c1 + 0.114 c2) - 1 (not clamped);  u = ((2x - 1 + 1) / 2)(GW - 1), v likewise with y, GH,
 *        w = ((z + 1) / 2)(L - 1), each clamped to [0, size - 1] (evaluated in fp64 as x (GW - 1), y (GH - 1), gray (L - 1));
 *        A_k = trilinear sample of grids[idx_b][k] at (w, v, u);
 *        out_i = sum_{j<3} A_{4i+j} c_j + A_{4i+3}.
 *  gspl_bilagrid_slice_bwd: grad_rgb (nullable) dc_j = sum_i dout_i A_{4i+j} + (L - 1) wgt_j sum_k dA_k (B_k(z0+1) - B_k(z0)) with
 *      dA_{4i+j} = dout_i c_j, dA_{4i+3} = dout_i, B_k the bilinear sample at level z; the w term is 0 where w was clamped or lies
 *      on 0 or L - 1.  grad_grids (nullable) [N, 12, L, GH, GW], dense, every element written: the trilinear scatter of dA, zero for
 *      grids no image selects.  Deterministic, no float atomics: one workgroup per pixel block sums its pixels in a fixed order into
 *      a slab row (`workspace`, gspl_bilagrid_workspace_bytes(L, GH, GW, B, H, W) bytes, 16-byte aligned); a second kernel adds
 *      the rows covering each element in block order.  The workspace's contents on entry do not matter.
 *  gspl_bilagrid_tv_fwd: out[0] = (1/N) sum_d S_d / K_d over x [N, C, L, GH, GW], S_d the sum of squared neighbour differences
 *      along d, K_d = C (n_d - 1) prod_{e != d} n_e (a term with n_d = 1 is 0).  Two-level fixed-order sum over
 *      gspl_bilagrid_tv_partials(N C L GH GW) partials (f32 scratch).  gspl_bilagrid_tv_bwd: grad_x = grad_out[0] dTV/dx
 *      (grad_out on the device).
 * ---------------------------------------------------------------------------------------- */
size_t gspl_bilagrid_workspace_bytes(int L, int GH, int GW, int B, int H, int W);
int gspl_bilagrid_slice_fwd(int N, int L, int GH, int GW, int B, int H, int W, const float* grids, const float* xy, int64_t xy_bstride,
                            const float* rgb, int layout, const int32_t* idx, int idx_stride, float* out, void* stream);
int gspl_bilagrid_slice_bwd(int N, int L, int GH, int GW, int B, int H, int W, const float* grids, const float* xy, int64_t xy_bstride,
                            const float* rgb, int layout, const int32_t* idx, int idx_stride, const float* grad_out, int go_layout,
                            float* grad_grids /*nullable*/, float* grad_rgb /*nullable*/, int gr_layout, void* workspace,
                            size_t workspace_bytes, void* stream);
int gspl_bilagrid_tv_partials(int64_t n);
int gspl_bilagrid_tv_fwd(int N, int C, int L, int GH, int GW, const float* x, float* partials, float* out, void* stream);
int gspl_bilagrid_tv_bwd(int N, int C, int L, int GH, int GW, const float* x, const float* grad_out, float* grad_x, void* stream);

/* ------------------------------------------------------------------------------------------
 * 15. Normal maps from depth maps, the 2DGS maps and the surface regulariser sums (csrc/normals.hip).  PURELY ADDITIVE: seven new
 *    entry points, nothing existing changes, GSPL_ABI_VERSION stays 39.  fp32, device pointers only, no float atomics; every element
 *    of every output is written (hand over uninitialised memory); results are bit-reproducible.
 *
 *  The stencil.  rays [3,3] row-major (DEVICE memory) is a matrix A; r(y,x) = A (x, y, 1)^T, with normalize_rays r / max(|r|, 1e-12);
 *  q(y,x) = depth(y,x) r(y,x) (the camera origin cancels below and is left out).  For an interior pixel
 *        dx = q(y+1,x) - q(y-1,x),  dy = q(y,x+1) - q(y,x-1),  c = dx x dy,  n = c / max(|c|, 1e-12)        (F.normalize's rule)
 *  and n = 0 on the one-pixel border; H < 3 or W < 3 gives all zeros.  This is the 2DGS renderer's `depth_to_normal` (A = c2w[:3,:3]
 *  intrins^-1) and, with A = c2w[:3,:3] [[1/fx, 0, (0.5 - cx)/fx], [0, 1/fy, (0.5 - cy)/fy], [0, 0, 1]], gsplat's `utils.depth_to_normal`
 *  (normalize_rays = not z_depth).
 *  gspl_depth_normal_fwd: depth [H,W] -> normal, 3 H W floats in `layout` (GSPL_LAYOUT_HWC: [H,W,3], GSPL_LAYOUT_CHW: [3,H,W]).
 *  gspl_depth_normal_bwd: v_normal (in `layout`) -> v_depth [H,W], a gather: each pixel adds up, in a fixed order, what the four centres
 *      (y+-1,x), (y,x+-1) that read it contribute, recomputing their cross products from `depth` (a radius-2 diamond).  Where
 *      |c| <= 1e-12 the constant denominator is kept, v_c = v_n / 1e-12, as torch's F.normalize backward does: gradients there carry
 *      that 1e12 scale (and are exactly 0 where the depth map is exactly 0 around the pixel).
 *  gspl_surfel_maps_fwd: allmap [7,H,W] (planes: depth | alpha | view normal x3 | median depth | distortion), normal_rot [3,3] and
 *      rays [3,3] (device), rho = depth_ratio:
 *        rend_normal [3,H,W] = normal_rot allmap[2:5]
 *        surf_depth  [1,H,W] = (1 - rho) nan0(allmap0 / alpha) + rho nan0(allmap5),   nan0 = torch.nan_to_num(x, 0, 0): NaN, +inf -> 0,
 *                              -inf -> the lowest finite value
 *        surf_normal [3,H,W] = stencil(surf_depth) alpha                                (alpha is a constant of this product)
 *  gspl_surfel_maps_bwd: the three upstream gradients (each nullable = zero) -> v_allmap [7,H,W], written completely: plane 6 is 0;
 *      planes 2..4 = normal_rot^T v_rend_normal; with v = v_surf_depth + the stencil's gather, plane 0 = v (1 - rho) / alpha, plane 1 =
 *      -v (1 - rho) allmap0 / alpha^2 (from the expected depth only), plane 5 = v rho.  Planes 0 and 1 are 0 where allmap0 / alpha is
 *      not finite, plane 5 where allmap5 is not: nan0 passes no gradient there.  (torch's formulation leaves NaN in planes 0 and 1 at
 *      alpha = 0, from 0 / 0 in the division's backward; that is deliberately not reproduced.)
 *  gspl_surface_reg_fwd: a, b [3,H,W], dist [H,W] (nullable): out[0] = mean_p (1 - sum_c a_c b_c), out[1] = mean_p dist (0 without
 *      dist).  Deterministic: gspl_surface_reg_partials(H W) workgroups write 2 partial sums each to `partials` (2x as many floats),
 *      one workgroup adds them in a fixed order.  A thread adds at most 64 terms serially, a workgroup's tree is 9 additions deep,
 *      at both levels; 1 <= H W <= 2^28.
 *  gspl_surface_reg_bwd: grad_out [2] on the device -> v_a = -grad_out[0] b / (H W), v_b = -grad_out[0] a / (H W), v_dist =
 *      grad_out[1] / (H W); each output nullable (not written).
 * ---------------------------------------------------------------------------------------- */
int gspl_depth_normal_fwd(int H, int W, const float* depth, const float* rays, int normalize_rays, int layout, float* normal, void* stream);
int gspl_depth_normal_bwd(int H, int W, const float* depth, const float* rays, int normalize_rays, const float* v_normal, int layout,
                          float* v_depth, void* stream);
int gspl_surfel_maps_fwd(int H, int W, const float* allmap, const float* normal_rot, const float* rays, float depth_ratio,
                         float* rend_normal, float* surf_depth, float* surf_normal, void* stream);
int gspl_surfel_maps_bwd(int H, int W, const float* allmap, const float* normal_rot, const float* rays, float depth_ratio,
                         const float* v_rend_normal /*nullable*/, const float* v_surf_depth /*nullable*/,
                         const float* v_surf_normal /*nullable*/, float* v_allmap, void* stream);
int gspl_surface_reg_partials(int64_t n);
int gspl_surface_reg_fwd(int H, int W, const float* a, const float* b, const float* dist /*nullable*/, float* partials, float* out,
                         void* stream);
int gspl_surface_reg_bwd(int H, int W, const float* a, const float* b, const float* grad_out, float* v_a /*nullable*/,
                         float* v_b /*nullable*/, float* v_dist /*nullable*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * 16. Wide-feature compositing (csrc/features.hip).  PURELY ADDITIVE: two new entry points, nothing existing changes,
 *    GSPL_ABI_VERSION stays 39.  What Feature-3DGS (internal/renderers/feature_3dgs_renderer.py) and SegAnyGS
 *    (internal/renderers/gsplat_contrastive_feature_renderer.py) ask of a rasterizer: many channels per splat composited over a
 *    frozen model, and the gradient of the features alone.
 *
 *  Arguments as gspl_composite_fwd / gspl_composite_bwd (section 4) with these differences: any D >= 1; `features` [N,D];
 *  backgrounds [D] (nullable = zero); no hit flags.  n_isects < 0: `offsets` has tile_w tile_h + 1 entries, the last one the list
 *  length (gspl_bin_sort_device_count).  tile_size 8, 16 or 32 (else GSPL_ERR_UNSUPPORTED); D < 1, an unknown mode or layout, a
 *  tile grid that does not cover the image or a NULL required pointer: GSPL_ERR_INVALID_ARG, nothing is launched.
 *  gspl_feature_fwd: out ([H,W,D] in GSPL_LAYOUT_HWC, [D,H,W] in GSPL_LAYOUT_CHW), out_alphas, final_Ts, last_ids [H,W], every element
 *      written.  Per channel, out = the fmaf chain over the pixel's list in list order plus T background: bit-for-bit what
 *      gspl_composite_fwd gives for the same channel, and the same out_alphas / final_Ts / last_ids.  N == 0 or n_isects == 0: the
 *      background everywhere, alpha 0, T 1, last_ids 0; the splat and list pointers are not read (may be NULL).
 *  gspl_feature_bwd: v_features [N,D] += sum over pixels of (alpha T) v_out[pixel, :] — ZEROED BY THE CALLER, accumulated with fp32
 *      atomics (one per 8x8 pixel block, splat and channel; the order of the additions is not fixed, results are not
 *      bit-reproducible).  v_out in `layout`.  No other gradient is computed.  N == 0 or n_isects == 0: nothing is launched.
 * ---------------------------------------------------------------------------------------- */
int gspl_feature_fwd(int N, int64_t n_isects, int D, int mode, int layout,
                     const float* means2d, const float* conics, const float* features, const float* opacities,
                     const float* backgrounds /*nullable*/, int width, int height, int tile_size, int tile_w, int tile_h,
                     const int32_t* offsets, const int32_t* flatten_ids,
                     float* out, float* out_alphas, float* final_Ts, int32_t* last_ids, void* stream);
int gspl_feature_bwd(int N, int64_t n_isects, int D, int mode, int layout,
                     const float* means2d, const float* conics, const float* opacities,
                     int width, int height, int tile_size, int tile_w, int tile_h,
                     const int32_t* offsets, const int32_t* flatten_ids, const int32_t* last_ids,
                     const float* v_out, float* v_features, void* stream);

/* ------------------------------------------------------------------------------------------
 * 17. Periodic Vibration Gaussians: the vibration transform (csrc/pvg.hip) and the cube-map sky (csrc/envlight.hip).  PURELY
 *    ADDITIVE: six new entry points, nothing existing changes, GSPL_ABI_VERSION stays 39.  fp32, device pointers only; what
 *    internal/models/periodic_vibration_gaussian.py, internal/renderers/periodic_vibration_gaussian_renderer.py and
 *    internal/model_components/envlight.py compute with some fifteen elementwise launches, a direction grid and nvdiffrast.
 *
 *  The vibration transform.  Rows: means, velocity [N,3]; t, scale_t, opacities [N] (scale_t and opacities ACTIVATED, as the model's
 *  getters return them).  table (DEVICE memory, 6 floats): ts = camera time + time_offset - time_shift | time_shift | 1 when shifted
 *  else 0 | cycle | velocity_decay | a = 2 pi / cycle.
 *        avg_velocity = velocity exp(-scale_t / cycle / 2 velocity_decay)
 *        means_t      = means + velocity sin((ts - t) a) / a,  plus avg_velocity time_shift when shifted
 *        marginal     = exp(-0.5 (t - ts)^2 / scale_t^2),      opacity_t = opacities marginal
 *  gspl_pvg_motion_fwd: one launch, every element of means_t, avg_velocity [N,3] and opacity_t [N] written.  N == 0: no launch.
 *  gspl_pvg_motion_bwd: the three upstream gradients (each nullable = zero) -> g_means, g_velocity [N,3], g_t, g_scale_t,
 *      g_opacities [N], every element written, in one launch; sin, cos and exp are recomputed from the inputs.  Where marginal
 *      underflows to 0 (or is undefined) the terms through it are exactly 0: nothing is NaN or infinite there.
 *
 *  The cube map.  base [6,R,R,3] (face, row, column, channel), 1 <= R <= 8192; a direction l = (x, y, z):
 *    - zero or non-finite l: value 0, no gradient.
 *    - the major axis is x if |x| >= |y| and |x| >= |z|, else y if |y| >= |z|, else z; ma = |major component|; (sc, tc) per face:
 *        0 (+x): (-z, -y)   1 (-x): (+z, -y)   2 (+y): (+x, +z)   3 (-y): (+x, -z)   4 (+z): (+x, -y)   5 (-z): (-x, -y)
 *      s = (sc / ma + 1) / 2, t = (tc / ma + 1) / 2; texel coordinates x = s R - 0.5 (column), y = t R - 0.5 (row).
 *    - bilinear over the four taps around (x, y).  A tap one texel off the face in ONE coordinate is taken from the adjacent face:
 *      its centre on this face's extended plane is folded over the shared edge (the overflowing coordinate becomes +-1, the former
 *      major coordinate 1 - 1/R), and the face and nearest texel are selected again from the folded point.  A tap off the face in
 *      BOTH coordinates is a cube corner and has no texel: it is dropped and the other three weights are divided by their sum.
 *      R == 1 is legal.
 *    These are the published OpenGL / nvdiffrast (filter_mode='linear', boundary_mode='cube') semantics; parity with nvdiffrast's own
 *    build is UNPINNED (it cannot be built here); the fp64 restatement in tests/pvg_oracle.py pins this implementation.
 *  gspl_cubemap_fwd: dirs [M,3] -> out [M,3], every element written.
 *  gspl_cubemap_bwd: g_base [6,R,R,3] += weights v_out — ZEROED BY THE CALLER, fp32 atomics (the order of the additions is not
 *      fixed).  There is no gradient for the directions.
 *  gspl_envlight_blend_fwd: table (DEVICE, 13 floats): the camera-to-world rotation [3,3] row-major | fx | fy | cx | cy.  Per pixel
 *      (u, v): d = normalize(((u - cx + ju) / fx, (v - cy + jv) / fy, 1)) with (ju, jv) = jitter[:, v, u] (jitter [2,H,W], nullable
 *      = 0.5); l = swap(rotation d), swap(x, y, z) = (x, z, -y); out [3,H,W] = rgb + (1 - alpha) sample(l), rgb [3,H,W], alpha
 *      [H,W].  dirs_out [H,W,3] (nullable) receives l.
 *  gspl_envlight_blend_bwd: v_out [3,H,W] -> g_alpha [H,W] (nullable) = -sum_c v_out_c sample(l)_c, written; g_base (nullable,
 *      ZEROED BY THE CALLER) += weights (1 - alpha) v_out, fp32 atomics.  (The gradient of rgb is v_out itself.)  The direction
 *      and the taps are recomputed.
 * ---------------------------------------------------------------------------------------- */
int gspl_pvg_motion_fwd(int N, const float* means, const float* velocity, const float* t, const float* scale_t,
                        const float* opacities, const float* table, float* means_t, float* avg_velocity, float* opacity_t,
                        void* stream);
int gspl_pvg_motion_bwd(int N, const float* velocity, const float* t, const float* scale_t, const float* opacities,
                        const float* table, const float* v_means_t /*nullable*/, const float* v_avg_velocity /*nullable*/,
                        const float* v_opacity_t /*nullable*/, float* g_means, float* g_velocity, float* g_t, float* g_scale_t,
                        float* g_opacities, void* stream);
int gspl_cubemap_fwd(int64_t M, int R, const float* dirs, const float* base, float* out, void* stream);
int gspl_cubemap_bwd(int64_t M, int R, const float* dirs, const float* v_out, float* g_base, void* stream);
int gspl_envlight_blend_fwd(int H, int W, int R, const float* table, const float* rgb, const float* alpha, const float* base,
                            const float* jitter /*nullable*/, float* out, float* dirs_out /*nullable*/, void* stream);
int gspl_envlight_blend_bwd(int H, int W, int R, const float* table, const float* alpha, const float* base,
                            const float* jitter /*nullable*/, const float* v_out, float* g_alpha /*nullable*/,
                            float* g_base /*nullable*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * 18. Mesh extraction for the 2DGS route (csrc/mesh.hip): TSDF fusion of depth maps and marching tetrahedra.  PURELY ADDITIVE: three
 *    new entry points and one constant, nothing existing changes, GSPL_ABI_VERSION stays 39.  fp32 data, device pointers only, no
 *    atomics of any kind; every output is bit-reproducible.  What internal/utils/gs2d_mesh_utils.py (`extract_mesh_unbounded`) computes
 *    with some twenty launches and four masked scatters per camera and chunk, and a marching cubes on the CPU.
 *
 *  gspl_tsdf_fuse: the running average of V views at M samples, one launch, state updated in place.
 *    The samples.  points [M,3] when not NULL.  points == NULL: a block of a lattice that is never materialised.  The lattice has
 *      n = (n0, n1, n2) nodes, the block starts at node b = (b0, b1, b2) and has m = (m0, m1, m2) nodes (0 <= b, b + m <= n,
 *      M == m0 m1 m2); sample index ((i m1) + j) m2 + k, k fastest, is node g = b + (i, j, k), at
 *          s_a = fmaf((float)g_a, step_a, lo_a),  step_a = (hi_a - lo_a) / (float)(n_a - 1)     for n_a > 1,        s_a = lo_a for n_a == 1:
 *      the difference and the quotient rounded to fp32, then ONE rounding of lo + g step (in numpy: the float64 sum of lo and the exact
 *      float64 product, rounded to float32).  Blocks of one lattice therefore see bit-identical nodes on the planes they share, and a
 *      node is within half an ulp of its own value however much lo cancels.  With points the nine lattice integers are ignored.
 *    table (DEVICE memory, GSPL_TSDF_TABLE_FLOATS = 16 floats): center[3] | radius | voxel_size | sdf_trunc (<= 0: 5 voxel_size) |
 *      depth_trunc (<= 0: none) | contract (0 or 1) | with_rgb (0 or 1) | lo[3] | hi[3] | 0.
 *    view_table [V,16]: each view's full projection, row-major, ROW-VECTOR convention (p = (x, 1) P, as the reference's cameras hold
 *      `full_projection`); depth [V,H,W]; rgb [V,3,H,W] (nullable).  State: tsdf [M], weight [M], color [M,3] (nullable).  Colour is
 *      fused when the table's with_rgb is set AND rgb and color are both not NULL; otherwise color is neither read nor written.
 *    Per sample s:
 *      contract:  mag = |s|;  T = sdf_trunc, times 1 / (2 - min(mag, 1.9)) where mag > 1;  u = s where mag < 1, else
 *                 (1 / (2 - mag)) (s / mag);  x = u radius + center.        Without contract: x = s, T = sdf_trunc.
 *      for v = 0 .. V-1, in this order:
 *        p = (x, 1) P_v,  z = p.w,  pix = p.xy / p.w;  the view counts if -1 < pix.x, pix.y < 1 and z > 0;
 *        d = the bilinear sample of depth_v at pix, align_corners=True, border padding: ix = (pix.x + 1) / 2 (W - 1) clamped to
 *            [0, W-1], x0 = floor(ix), x1 = min(x0 + 1, W - 1), likewise in y (valid for W == 1 or H == 1: the one tap);
 *        it further needs d - z > -T and, with depth_trunc > 0, 0 < d <= depth_trunc.  (The depth_trunc cut is the bounded mode's; it
 *            is NOT in the reference's torch path, which Open3D's integration applies to its depth images instead.)
 *        if it counts:  tsdf = (tsdf w + clamp((d - z) / T, -1, 1)) / (w + 1);  color likewise with the same taps of rgb_v;  w += 1.
 *      Everything up to and including the clamped quotient (and the colour sample) is evaluated in fp64 from the fp32 inputs and rounded
 *      to fp32 once; the average is fmaf(tsdf, w, value) / (w + 1) in fp32.  The kernel CONTINUES from the state it is given: the
 *      caller initialises tsdf = 1, weight = 1, color = 0 as the reference does, and fusing views [0, a) and then [a, V) in two calls
 *      gives the bits of one call (cameras of several image sizes, or a bounded map stack, are fused stack by stack).
 *    M == 0 or V == 0: no launch, returns 0, the state is untouched.  One thread per sample, 64-bit indexing throughout
 *    (V H W and 3 M may pass 2^31).  A NaN or infinite projection fails the pixel test: the view does not count and nothing is read.
 *
 *  gspl_mtet_count / gspl_mtet_emit: the iso-surface of volume [X,Y,Z] (k fastest) by marching tetrahedra.  No case table, no
 *    ambiguous case, and a closed 2-manifold wherever the surface does not leave the volume.
 *    Decomposition.  Cell (i, j, k), i < X-1, j < Y-1, k < Z-1, with first corner v0 = (i, j, k), is cut into the six Kuhn
 *      tetrahedra: for the permutations (a, b, c) of the axes (0, 1, 2) in lexicographic order, corners v0, v0 + e_a, v0 + e_a + e_b,
 *      v0 + e_a + e_b + e_c.  The same under every translation: neighbouring cells agree on the faces they share.
 *    Inside.  A corner is inside iff value < level (a NaN is outside).
 *    Cases.  Stable-partition the four corners, inside ones first, and name them 0..3.  One inside corner: the triangle on edges
 *      (0,1) (0,2) (0,3); three: (0,3) (1,3) (2,3); two: (0,2) (0,3) (1,3) and then (0,2) (1,3) (1,2).  A triangle has its last two
 *      vertices swapped when its normal points from the centroid of the outside corners towards the centroid of the inside ones;
 *      the test is exact, in integers, on the edge midpoints of the unit cell (it is the same for every crossing point and every
 *      positive step).  Normals point from inside to outside: a closed surface around an inside region has positive signed volume.
 *    Vertices.  A vertex lies on a lattice edge between nodes A and B, A the one with the lower global linear index whichever is
 *      inside:  t = (level - f_A) / (f_B - f_A),  p_a = fmaf(t, pB_a - pA_a, pA_a),  pN_a = fmaf((float)node_a, step_a, origin_a) with
 *      the GLOBAL node index: every triangle of every block that uses the edge computes the same bits, and with origin = lo,
 *      step = (hi - lo) / (n - 1) a node lies where gspl_tsdf_fuse's lattice put it.  grid (DEVICE memory, 6 floats): origin[3] of
 *      global node 0 | step[3], step > 0.
 *    Keys.  key = global_linear_index(A) * 8 + direction, int64; the global index is ((g_0 G1) + g_1) G2 + g_2 with g = b + local node
 *      and the caller's global dimensions G = (g0, g1, g2) and block offset b (0 <= b, b + (X, Y, Z) <= G); direction of B - A:
 *      (1,0,0) 0, (0,1,0) 1, (0,0,1) 2, (1,1,0) 3, (1,0,1) 4, (0,1,1) 5, (1,1,1) 6.  Blocks that share a plane give equal keys on it.
 *    gspl_mtet_count: counts [(X-1)(Y-1)(Z-1)] u8, cell-major (k fastest): the cell's triangles, at most 12.
 *    gspl_mtet_emit: offsets = the EXCLUSIVE prefix sum of counts (int32), total = its end (the one number the host reads) ->
 *      vertices [3 total, 3] and keys [3 total], triangle after triangle: cell-major, then the tetrahedra in the order above, then the
 *      triangles in the order above.  A cell whose offset and count do not fit [0, total] writes nothing.
 *    X, Y or Z < 2, or total == 0: no launch, returns 0.
 * ---------------------------------------------------------------------------------------- */
#define GSPL_TSDF_TABLE_FLOATS 16
int gspl_tsdf_fuse(int64_t M, const float* points /*nullable*/, int n0, int n1, int n2, int b0, int b1, int b2, int m0, int m1, int m2,
                   const float* table, int V, int H, int W, const float* view_table, const float* depth, const float* rgb /*nullable*/,
                   float* tsdf, float* weight, float* color /*nullable*/, void* stream);
int gspl_mtet_count(int X, int Y, int Z, const float* volume, float level, uint8_t* counts, void* stream);
int gspl_mtet_emit(int X, int Y, int Z, const float* volume, float level, const float* grid, int g0, int g1, int g2,
                   int b0, int b1, int b2, const int32_t* offsets, int64_t total, float* vertices, int64_t* keys, void* stream);

/* ------------------------------------------------------------------------------------------
 * 19. K nearest neighbours and local feature smoothing for the SegAnyGS route (csrc/knn.hip, csrc/smooth.hip).  PURELY ADDITIVE: six
 *    new entry points, nothing existing changes (section 7 keeps its results), GSPL_ABI_VERSION stays 39.  fp32 data, device
 *    pointers only.  What `pytorch3d.ops.knn_points` and the gather / mean of internal/segany_splatting.py:262-309 compute (the latter
 *    through an [N, S, D] tensor), and what internal/metrics/appearance_feature_similarity_regularization_metrics.py:70-74 queries.
 *
 *  gspl_knn_points: for each of the P1 queries p1 [P1,3] the K (1 <= K <= 32) nearest of the P2 reference points p2 [P2,3], exact.
 *    dists [P1,K] f32: squared Euclidean distances as the kernel's fp32 arithmetic gives them, ascending; idx [P1,K] i64 into p2.
 *    Order: by (d^2, index) — among equal fp32 d^2 the lower index first; the output is the same bits on every run.  A query that
 *    coincides with a reference point finds it at distance 0 (p1 == p2: every point is its own first neighbour).  Queries may lie
 *    anywhere, also far outside the reference cloud.  A reference point with a non-finite coordinate is never returned; where fewer
 *    than K finite reference points exist the trailing entries of both rows are 0.  A query with a non-finite coordinate gets a row
 *    of zeros (the call terminates; pytorch3d leaves such a row unspecified).  workspace: gspl_knn_points_workspace_bytes(P2).
 *    P1 == 0: no launch.  P2 == 0: rows of zeros.
 *
 *  gspl_knn_graph: the inverse adjacency of a neighbour map idx [N,K] i32 (values 0 .. N-1; anything else is ignored) in CSR form:
 *    entries [N K] u32 holds, for row j at [row_start[j], row_start[j+1]), the positions e = i K + k with idx[i,k] == j, ascending
 *    (i.e. sorted by (i, k)); row_start [N+1] u32.  Built with a count, the exclusive scan and the stable radix sort of section 10:
 *    deterministic.  The tail of `entries` behind row_start[N] is unspecified.  N K < 2^30.
 *
 *  gspl_smooth_features_fwd / _bwd: features [N,D] (1 <= D <= 128), idx [N,K] i32 with values 0 .. N-1 (NOT checked: the caller
 *    validates the map once, when it builds the graph), mask: bit k set = column k of idx takes part (not 0, no bit >= K), S = its
 *    population count.
 *      n_j = x_j / max(|x_j|, 1e-12);   m_i = (1 / S) sum over the selected k of n_idx[i,k];   out_i = m_i / (|m_i| + 1e-9)
 *    fwd writes out [N,D] and mnorm [N] = |m_i| (the backward needs it), one launch.  bwd: v_features [N,D] = dL/dfeatures from
 *    v_out [N,D], one launch over the inverse adjacency of the same idx, no atomics, the same bits on every run; it follows torch's
 *    subgradients at the two guards (|m| == 0: no gradient through |m|; |x| < 1e-12: v_x = v_n / 1e-12).
 * ---------------------------------------------------------------------------------------- */
size_t gspl_knn_points_workspace_bytes(int P2);
int gspl_knn_points(int P1, const float* p1, int P2, const float* p2, int K, float* dists, int64_t* idx,
                    void* workspace, size_t workspace_bytes, void* stream);
size_t gspl_knn_graph_workspace_bytes(int N, int K);
int gspl_knn_graph(int N, int K, const int32_t* idx, uint32_t* row_start, uint32_t* entries,
                   void* workspace, size_t workspace_bytes, void* stream);
int gspl_smooth_features_fwd(int N, int D, int K, uint32_t mask, const float* features, const int32_t* idx, float* out, float* mnorm,
                             void* stream);
int gspl_smooth_features_bwd(int N, int D, int K, uint32_t mask, const float* features, const uint32_t* row_start, const uint32_t* entries,
                             const float* out, const float* mnorm, const float* v_out, float* v_features, void* stream);

/* ------------------------------------------------------------------------------------------
 * 20. Multiresolution hash-grid / dense-grid encoding for the SWAG route (csrc/hashgrid.hip).  PURELY ADDITIVE: two new entry
 *    points, no new struct, nothing existing changes, GSPL_ABI_VERSION stays 39.  What `tinycudann.Encoding` with otype HashGrid or
 *    DenseGrid and linear interpolation computes (internal/models/swag_model.py:75-78,98).  PARITY UNPINNED: there is no ROCm build of
 *    tiny-cuda-nn to compare against; these are its published rules, and the fp64 oracle tests/hashgrid_oracle.py pins them here.
 *
 *  x [N,D] f32 (D = 2 or 3), F = 1, 2, 4 or 8 features per level, L = 1 .. 32 levels, table [offsets[L], F] f32, level-major.
 *  The level table is computed ONCE ON THE HOST, in double, rounded once, and passed as HOST arrays (`ops.hashgrid_levels`):
 *      scales[l]      = float32(exp2(l log2(per_level_scale)) base_resolution - 1)
 *      resolutions[l] = ceil(scales[l]) + 1
 *      size_l         = min(resolutions[l]^D, (2^32 - 1) / 2) rounded up to a multiple of 8; HashGrid: also capped at 2^log2_hashmap_size
 *      offsets[l]     = running sum of the sizes ([L + 1]; offsets[l + 1] - offsets[l] = size_l <= 2^31, offsets[L] < 2^32)
 *  A level is hashed iff resolutions[l]^D > size_l (derived here from the two arrays).
 *  Per point and level:  pos_d = fmaf(x_d, scale_l, 0.5f) (ONE rounding);  cell_d = floor(pos_d) converted through int32 to uint32,
 *  so negative and far inputs are legal and wrap;  frac_d = pos_d - floor(pos_d).  For each of the 2^D corners c (bit d of c selects
 *  cell_d + 1): weight = product over d of (bit ? frac_d : 1 - frac_d); row = sum_d corner_d resolutions[l]^d (dense) or the XOR over d
 *  of corner_d prime_d with primes (1, 2654435761, 805459861) (hashed), both in uint32, then mod size_l.
 *      out[n, l F + f] = sum over corners of weight table[offsets[l] + row, f]
 *  Every row index is reduced mod size_l, so no input value can address outside the table.
 *
 *  gspl_hashgrid_fwd: out [N, L F].  One launch, one level per blockIdx.y.
 *  gspl_hashgrid_bwd: v_out [N, L F].  v_table (nullable) [offsets[L], F] is ACCUMULATED into (the caller clears it) with fp32
 *    atomics: the sum depends on arrival order in the last bits.  Lanes of a wave whose consecutive points share a destination row are
 *    summed before the atomic.  v_x (nullable; needs `table`) [N,D] is WRITTEN, without atomics:
 *      v_x[n,d] = sum_l scale_l sum over corners of (+-1 on d) (product of the other dims' weights) <table row, v_out[n, l F ..]>
 *    A (point, level) whose F values of v_out are all zero contributes nothing and is skipped before it reads x or the table.
 *  table, out and v_out must be aligned to a row (4 F bytes, 16 from F = 4).  N == 0: no launch.
 * ---------------------------------------------------------------------------------------- */
int gspl_hashgrid_fwd(int N, int D, int F, int L, const float* scales, const uint32_t* resolutions, const uint32_t* offsets,
                      const float* x, const float* table, float* out, void* stream);
int gspl_hashgrid_bwd(int N, int D, int F, int L, const float* scales, const uint32_t* resolutions, const uint32_t* offsets,
                      const float* x, const float* table, const float* v_out, float* v_table, float* v_x, void* stream);

/* ------------------------------------------------------------------------------------------
 * 21. The per-Gaussian appearance MLP of the appearance-embedding route, fused (csrc/appearance.hip).  PURELY ADDITIVE: three new
 *    entry points, no new struct, nothing existing changes, GSPL_ABI_VERSION stays 39.  What `Model.forward` of
 *    internal/renderers/gsplat_appearance_embedding_renderer.py computes with `tcnn: false`, for the ONE embedding row of a call.
 *    The reference's arithmetic is torch code, so it is pinned directly (tests/appearance_oracle.py); exact fp32 on the f32-input MFMA.
 *
 *  features [N,F] f32, F % 4 == 0, 4 <= F <= 128; embedding [E] f32, E <= 256; H = 32 or 64 hidden neurons; n_layers = 2 .. 4 linear
 *  layers; n_out = 3 or 4; n_freq = 0 .. 8.  `weights` and `biases` are HOST arrays of n_layers DEVICE pointers in torch.nn.Linear
 *  layout: weights[l] [out_l, in_l], biases[l] [out_l]; in_0 = F + E + P with P = n_freq ? 3 (2 n_freq + 1) : 0, the columns in the
 *  order features | embedding | encoded direction; in_l = H after that; out_l = H but for the last, n_out.
 *  flags: 1 = F.normalize (eps 1e-12) on each feature row and on the embedding; 2 = sigmoid on the output (else none).
 *  n_freq > 0: d = (means[n] - camera_center) / max(|.|, 1e-12) (means [N,3], camera_center [3], both on the device), encoded as
 *  d, sin(2^0 d), cos(2^0 d), sin(2^1 d), ...; d carries no gradient.  mask (nullable) [N] bytes: rows with 0 are not evaluated.
 *      x = [f^ | e^ | enc(d)];  a_0 = relu(W_0 x + b_0);  ...;  out = act(W_last a + b_last)
 *  The embedding is folded into the first bias once per workgroup: b_0' = b_0 + W_0[:, F:F+E] e^.
 *
 *  gspl_appearance_mlp_fwd: out [N, n_out], every row WRITTEN (masked rows: zeros).
 *  gspl_appearance_mlp_bwd: v_out [N, n_out] (masked rows are not read).  v_features (nullable) [N,F], 16-byte aligned: every row
 *    WRITTEN (masked rows: zeros).  v_params (nullable): the gradients in the parameters' own layout, every element WRITTEN,
 *        [W_0 | b_0 | W_1 | b_1 | ... | embedding [E]]
 *    Hidden activations are recomputed.  Rows are assigned to workgroups statically, each workgroup writes one partial into
 *    `workspace` (gspl_appearance_mlp_workspace_bytes), and a second launch sums the partials in workgroup order: no float atomics,
 *    the same bits on every run.  v_params == NULL: no weight-gradient arithmetic, no second launch, no workspace.
 *  A network whose LDS images do not fit 160 KiB is refused.  N == 0: no launch (v_params is cleared).
 * ---------------------------------------------------------------------------------------- */
size_t gspl_appearance_mlp_workspace_bytes(int N, int F, int E, int H, int n_layers, int n_out, int n_freq);
int gspl_appearance_mlp_fwd(int N, int F, int E, int H, int n_layers, int n_out, int n_freq, int flags, const float* features,
                            const uint8_t* mask, const float* means, const float* camera_center, const float* embedding,
                            const float* const* weights, const float* const* biases, float* out, void* stream);
int gspl_appearance_mlp_bwd(int N, int F, int E, int H, int n_layers, int n_out, int n_freq, int flags, const float* features,
                            const uint8_t* mask, const float* means, const float* camera_center, const float* embedding,
                            const float* const* weights, const float* const* biases, const float* v_out, float* v_features,
                            float* v_params, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * 22. The HexPlane / K-Planes field of the 4D-GS route (csrc/hexplane.hip).  PURELY ADDITIVE: two new entry points, no new struct,
 *    nothing existing changes, GSPL_ABI_VERSION stays 39.  What `HexPlaneField.forward` of
 *    internal/model_components/gs4d_hexplane.py computes with six `F.grid_sample` calls per level (bilinear, align_corners=True,
 *    padding_mode='border'), a product chain and a cat.  The reference's arithmetic is torch code, so it is pinned directly
 *    (tests/hexplane_oracle.py against tests/golden/ref_hexplane.npz).
 *
 *  x [N,3] f32; t [N] f32 per point, or NULL and ONE value `t_uniform` for the call; F = 8, 16, 32 or 64 features; L = 1 .. 8 levels.
 *  HOST arrays (`ops.hexplane_layout`):
 *      resolutions [L,4]  R_x, R_y, R_z, R_t of each level (the level's multiplier applies to the three spatial axes only), 1 .. 32768
 *      offsets [6 L + 1]  first row of plane p of level l at [6 l + p]; offsets[6 L] = rows of the table < 2^31
 *      box [6]            aabb[0] (the reference keeps the MAXIMUM corner there), then float32(2 / (aabb[1] - aabb[0]))
 *  The six planes of a level are the pairs (a, b) of itertools.combinations(range(4), 2): xy, xz, xt, yz, yt, zt.  Plane (a, b) has
 *  R_a R_b rows of F floats, CHANNEL-LAST, row = i_b R_a + i_a (the reference's parameter [1, F, R_b, R_a] with the channels moved
 *  last: a corner is one contiguous row).  offsets must give every plane exactly R_a R_b rows.
 *  Per point:  p = ((x - aabb[0]) scale - 1 per axis, t): the time is used as it comes.  Per axis of a level, in float32, each
 *  operation rounded once and none contracted:
 *      i = ((c + 1) / 2) (R - 1), clamped to [0, R - 1];  i0 = floor(i);  weights (1 - f, f) with f = i - i0
 *  A corner with index R (only when i == R - 1) contributes nothing.
 *      out[n, l F + f] = product over the six planes of (sum over the four corners of weight table[row, f])
 *
 *  gspl_hexplane_fwd: out [N, L F].  One launch, one level per blockIdx.y.
 *  gspl_hexplane_bwd: v_out [N, L F].  v_table (nullable), the table's shape, is ACCUMULATED into (the caller clears it) with fp32
 *    atomics, one float per lane and whole rows per wave-instruction: the sum depends on arrival order in the last bits.  A
 *    (point, level) whose F values of v_out are all zero adds nothing and is skipped before it reads x or the table.
 *    v_x (nullable) [N,3] is WRITTEN, without atomics; an axis whose unclamped i is not strictly inside (0, R - 1) gets no gradient
 *    from that level, as grid_sample's border padding has it.  There is no gradient for t.
 *  table, out and v_out must be aligned to 16 bytes.  N == 0: no launch.
 * ---------------------------------------------------------------------------------------- */
int gspl_hexplane_fwd(int N, int F, int L, const uint32_t* resolutions, const uint32_t* offsets, const float* box,
                      const float* x, const float* t, float t_uniform, const float* table, float* out, void* stream);
int gspl_hexplane_bwd(int N, int F, int L, const uint32_t* resolutions, const uint32_t* offsets, const float* box,
                      const float* x, const float* t, float t_uniform, const float* table, const float* v_out,
                      float* v_table, float* v_x, void* stream);

/* ------------------------------------------------------------------------------------------
 * 23. The SpotLessSplats route outside the rasterizer (csrc/spotless.hip).  PURELY ADDITIVE: seven new entry points, no new struct,
 *    nothing existing changes, GSPL_ABI_VERSION stays 39.  What `SpotLessMetricsModule` of internal/metrics/spotless_metrics.py
 *    computes in `mlp_mask`, `robust_mask`, `update_running_stats` (its histogram) and its masked L1.  The reference's arithmetic is
 *    torch code, so it is pinned directly (tests/spotless_oracle.py against tests/golden/ref_spotless.npz).  fp32, device pointers only,
 *    no float atomics: every float sum is taken in a fixed order, the same bits on every run.
 *
 *  The mask predictor.  The first linear layer is folded through the bilinear resampling by the caller (gspl_amd.spotless):
 *      G [h0, w0, 16] channel-last = W1[:, :C] sf at the feature map's own resolution;  A [mh, 16] = pe_y W1[:, C:C+40]^T + b1;
 *      B [mw, 16] = pe_x W1[:, C+40:]^T;  w2 [16], b2 [1] the second layer.  16 hidden units only.
 *      z[i, j, :] = bilinear(G)[i, j, :] + A[i, :] + B[j, :];   mask[i, j] = sigmoid(b2 + sum_c w2[c] relu(z[i, j, c]))
 *  H == W == 0: out [mh, mw] is the mask.  Otherwise out [H, W] is the mask resampled bilinearly once more, the network evaluated at
 *  the four source pixels of every output pixel; the mask itself is not written.
 *  Both resamplings follow F.interpolate(mode="bilinear", align_corners=False), no antialiasing; per axis, in float32:
 *      src = max(fma(I / O, o + 0.5, -0.5), 0);  i0 = floor(src);  i1 = min(i0 + 1, I - 1);  weights (1 - l, l) with l = src - i0
 *  The product and the sum of src are ONE fused operation, as torch's CPU and GPU kernels have it (their weights, read out with
 *  one-hot inputs, equal this rule's bit for bit and differ from the unfused one); every other operation is rounded on its own.
 *  and a sample is  (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11).
 *  Every dimension is 2 .. 16384 (the reference's positional encoding divides by height - 1).  G, A, B and the workspace must be
 *  aligned to 16 bytes.
 *
 *  gspl_spotless_mask_fwd: one launch.
 *  gspl_spotless_mask_bwd: v_out in the shape of out -> v_G, v_A, v_B in the shapes of G, A, B and v_w [17] (v_w2, then v_b2), every
 *    element WRITTEN.  v = the adjoint of the second resampling of v_out (gathered, when there is one); dy = v s (1 - s);
 *    dz = dy w2 [z > 0]; v_A the row sums of dz, v_B its column sums, v_G its adjoint bilinear, v_w2 = sum dy relu(z), v_b2 = sum dy.
 *    Hidden activations are recomputed.  Two launches: one wave per (64 mask columns, row of G) leaves partial sums in `workspace`
 *    (gspl_spotless_mask_workspace_bytes), the second adds them in index order.  A pixel with v == 0 is not evaluated.
 *
 *  gspl_spotless_error_stats: render, gt [3, H, W]; thresholds [2] (lower, upper) on the DEVICE; edges [bins + 1] on the device, the
 *    float32 linspace(0, 1, bins + 1); 1 <= bins <= 15360.  One launch writes
 *      err [H, W] = ((|d0| + |d1|) + |d2|) / 3 with a true division;
 *      counts [bins] int32, ADDED to (the caller clears it): torch.histogram's rules over (0, 1) — bin k holds edges[k] <= v <
 *        edges[k + 1], the last bin includes 1, values outside [0, 1] and NaN are dropped; integer atomics on a histogram in LDS;
 *      lower_mask, upper_mask [H, W]: 1 where err < threshold (strictly) at the pixel, or at 5 or more of the 9 pixels of its
 *        zero-padded 3 x 3 neighbourhood; else 0.
 *
 *  gspl_spotless_masked_l1_fwd: out [1] = sum_p mask[p] ((|d0| + |d1|) + |d2|) / (3 H W) by a fixed two-level sum; partials holds
 *    gspl_spotless_l1_partials(H W) floats.
 *  gspl_spotless_masked_l1_bwd: v_render [3, H, W] = sign(render - gt) grad_out[0] mask / (3 H W), rounded to float32 once, sign(0) = 0;
 *    grad_out on the device.
 * ---------------------------------------------------------------------------------------- */
int gspl_spotless_mask_fwd(int h0, int w0, int mh, int mw, int H, int W, const float* G, const float* A, const float* B,
                           const float* w2, const float* b2, float* out, void* stream);
size_t gspl_spotless_mask_workspace_bytes(int h0, int w0, int mh, int mw);
int gspl_spotless_mask_bwd(int h0, int w0, int mh, int mw, int H, int W, const float* G, const float* A, const float* B,
                           const float* w2, const float* b2, const float* v_out, float* v_G, float* v_A, float* v_B, float* v_w,
                           void* workspace, size_t workspace_bytes, void* stream);
int gspl_spotless_error_stats(int H, int W, int bins, const float* render, const float* gt, const float* thresholds, const float* edges,
                              float* err, int32_t* counts, float* lower_mask, float* upper_mask, void* stream);
int gspl_spotless_l1_partials(int64_t n);
int gspl_spotless_masked_l1_fwd(int H, int W, const float* render, const float* gt, const float* mask, float* partials, float* out,
                                void* stream);
int gspl_spotless_masked_l1_bwd(int H, int W, const float* render, const float* gt, const float* mask, const float* grad_out,
                                float* v_render, void* stream);

/* ------------------------------------------------------------------------------------------
 * 24. The SegAnyGS (SAGA) training step behind the renderer (csrc/segany.hip).  PURELY ADDITIVE: six new entry points, no new struct,
 *    nothing existing changes, GSPL_ABI_VERSION stays 39.  What `SegAnySplatting.mask_preprocess` and
 *    `forward_with_loss_calculation` of internal/segany_splatting.py compute after the choice of the sampled pixels.  The reference's
 *    arithmetic is torch code, so it is pinned directly (tests/segany_loss_oracle.py against tests/golden/ref_segany_loss.npz).  fp32 and
 *    integers, device pointers only.
 *
 *  Limits, checked by every entry point (GSPL_ERR_INVALID_ARG):  S sampled pixels 1 .. 4096 (every count is then <= 2^24, exact in
 *  float32);  N masks 1 .. 1024 (NW = ceil(N / 64) words, at most 16);  Ns scales 1 .. 16 (the reference has 10);  C a multiple of 4,
 *  4 .. 64 (the route's value is 32);  every image dimension 1 .. 16384.
 *
 *  gspl_segany_mask_stats: masks [N, H, W], one byte per entry (non-zero = inside), read ONCE.  Two launches write
 *      area [N] int32, ADDED to (the caller clears it): pixels per mask, integer atomics;
 *      cover [H, W] int32: how many masks hold the pixel;
 *      mean_size [H, W] = (sum_i mask_i(p) area_i) / (cover + 1e-9): the numerator exact in 64-bit integers and rounded once;
 *      packed [NW, H W] u64 (the caller's scratch): the membership words of every pixel in the masks' own order.
 *  gspl_segany_pack_membership: order [N] int32 (the permutation that sorts the masks' scales descending), pixel_index [S] int32 (flat
 *      indices into H W) -> bits [S, NW] u64: bit i of word w = mask order[64 w + i] holds the pixel.  An index outside the image, or
 *      an entry of `order` outside 0 .. N - 1, sets no bit.
 *
 *  gspl_segany_pair_labels: scale_index [Ns] int32 (the reference's `sampled_scale_index`, entry 0 holding -1; values are clamped to
 *      -1 .. 64 NW - 1), upper [Ns] u8 (the `upper_bound` flag of each sampled scale), head [Ns, S] int32 (scratch) ->
 *      labels [S, S] u16, BOTH triangles and the diagonal written: bit n = gt_corrs[n, h, j], by the closed form of the reference's loop
 *          head_n(p) = the largest i <= scale_index[n] with bit i of p set, or -1
 *          label_n(h, j) = (head_n(h) == head_n(j) >= 0)  OR  (bits_h & bits_j & {i > scale_index[n]}) != 0
 *          an upper scale: label_n(h, j) = (bits_h & bits_j) != 0
 *      counts [3] int32, ADDED to (the caller clears it), over the FULL S x S matrix: pairs labelled 1 at no scale, at every scale, and
 *      the rest (the reference's consistent_negative, consistent_positive, inconsistent).  Integer atomics: exact in any order.
 *
 *  gspl_segany_loss_fwd: rendered [C, Hr, Wr]; pixel_index [S] into the mh x mw grid of the masks, raster order; gates [Ns, C];
 *      labels, counts as above; a [S] > 0 (mean_size at the sampled pixels); rnd [S, S] (the reference's rand_like draw).
 *      F [S, C] (written; the backward reads it): the bilinear sample of `rendered` at the centre of each mask pixel by the rule of
 *        section 23 (F.interpolate, align_corners=False); the map at mask size is never made.  An index outside the grid gives zeros.
 *      X_n[s] = (F[s] * gates[n]) / max(||F[s] * gates[n]||, 1e-12);  corr_n(h, j) = X_n[h] . X_n[j], ONE fmaf chain over c from 0,
 *        symmetric in (h, j) by construction.
 *      w(h, j) = (max(P / (a_h a_j), 1) - 1) / (R - 1) * 9 + 1 with P = fl(a_max a_max), R = max(P / fl(a_min a_min), 1), every operation
 *        rounded to float32 on its own: bit-equal to the reference's min-max normalised matrix (NaN when R == 1, as there).
 *      Over h < j:  t+ = (float(counts[2]) / 2) / float(counts[1]),  t- the same with counts[0];
 *        M+ : (label 1 at every scale AND rnd < t+) OR any_n(corr_n < 0.75 AND label_n) OR inconsistent
 *        M- : (label 1 at no scale AND rnd < t-)    OR any_n(corr_n > 0.5 AND NOT label_n) OR inconsistent
 *      selected [S, S] u8: bit 0 = in M+, bit 1 = in M-; written for h < j only (the caller clears the rest).
 *      out [3]: loss = -sum_{M+} w sum_n label_n corr_n / (Ns |M+|) + sum_{M-} w sum_n (1 - label_n) relu(corr_n) / (Ns |M-|);
 *        cosine_pos, cosine_neg = the means of corr_n over ALL (n, h, j) of the full matrix with label 1 / label 0.  IEEE throughout:
 *        an empty selection gives 0 / 0 = NaN.  sel_counts [2] int32 = |M+|, |M-|.
 *      weight: NULL, or [S, S], every element written with w(h, j) (for tests).
 *      No float atomics: one partial per 16 x 16 tile of pairs, added in tile order in float64: two runs give the same bits.
 *  gspl_segany_loss_bwd: grad_out [1] on the device.  k_n(h, j) = grad_out [-w label_n / (Ns |M+|) [in M+]
 *      + w (1 - label_n) [corr_n > 0] / (Ns |M-|) [in M-]];  dX_n[h] = sum_j k_n(h, j) X_n[j] over both triangles, j in index order; through
 *      the normalisation (below its clamp the denominator is the constant 1e-12) to
 *      v_F [S, C] and v_gates [Ns, C] (summed over s in a fixed order), both WRITTEN, the same bits on every run.  corr is recomputed
 *      from F and gates; `selected` and `sel_counts` are the forward's; no [Ns, S, S] array is ever written.
 *      v_rendered: NULL, or [C, Hr, Wr], ACCUMULATED into (the caller clears it): the adjoint of the bilinear sample of v_F, by fp32
 *      atomics because samples share texels.  This scatter is OUTSIDE gspl_set_deterministic: its sums depend on arrival order in the
 *      last bits, as gspl_hexplane_bwd's v_table does.
 *  workspace: gspl_segany_loss_workspace_bytes(S, C, Ns) bytes for either call, aligned to 256 bytes (0: arguments out of range).
 * ---------------------------------------------------------------------------------------- */
int gspl_segany_mask_stats(int N, int H, int W, const uint8_t* masks, int32_t* area, int32_t* cover, float* mean_size,
                           uint64_t* packed, void* stream);
int gspl_segany_pack_membership(int N, int H, int W, int S, const uint8_t* masks, const int32_t* order, const int32_t* pixel_index,
                                uint64_t* bits, void* stream);
int gspl_segany_pair_labels(int S, int N, int Ns, const uint64_t* bits, const int32_t* scale_index, const uint8_t* upper, int32_t* head,
                            uint16_t* labels, int32_t* counts, void* stream);
size_t gspl_segany_loss_workspace_bytes(int S, int C, int Ns);
int gspl_segany_loss_fwd(int S, int C, int Ns, int Hr, int Wr, int mh, int mw, const float* rendered, const int32_t* pixel_index,
                         const float* gates, const uint16_t* labels, const int32_t* counts, const float* a, const float* rnd,
                         float* F, float* out, int32_t* sel_counts, uint8_t* selected, float* weight, void* workspace,
                         size_t workspace_bytes, void* stream);
int gspl_segany_loss_bwd(int S, int C, int Ns, int Hr, int Wr, int mh, int mw, const int32_t* pixel_index, const float* gates,
                         const uint16_t* labels, const float* a, const uint8_t* selected, const int32_t* sel_counts, const float* F,
                         const float* grad_out, float* v_F, float* v_gates, float* v_rendered, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * 25. The view-dependent opacity of the Glossy-Gaussian route (csrc/glossy.hip).  PURELY ADDITIVE: two new entry points, no new
 *    struct, nothing existing changes, GSPL_ABI_VERSION stays 39.  What `GlossyRendererModule.get_opacities`
 *    (internal/renderers/glossy_renderer.py) and `GlossyGaussianModel.get_view_dep_opacities` (internal/models/glossy_gaussian.py)
 *    compute: a one-channel spherical-harmonics expansion evaluated at the normalised view direction.  The reference's arithmetic is
 *    torch code, so it is pinned directly (tests/glossy_oracle.py against tests/golden/ref_glossy.npz).  fp32, device pointers only.
 *
 *  means [N, 3], origin [3] (on the device), dc [N], rest [N, n_rest] (NULL if and only if n_rest == 0), degree 0 .. 4,
 *  (degree + 1)^2 - 1 <= n_rest <= 61; anything else, or a NULL required pointer: GSPL_ERR_INVALID_ARG, nothing is launched.
 *  N == 0 succeeds without a launch.
 *      d = (means[n] - origin) / max(||means[n] - origin||, 1e-12)          (F.normalize: a splat AT the origin has d = 0, not NaN)
 *      raw = C0 dc[n] + sum_{k = 1}^{(degree + 1)^2 - 1} basis_k(d) rest[n, k - 1] + 0.5
 *      opacities[n] = min(max(raw, 0), 1)
 *  basis_k: the polynomials of internal/utils/sh_utils.py `eval_sh_decomposed`, evaluated as written there also where d is not a
 *  unit vector (at d = 0 the degree-4 term C4[4] (zz (35 zz - 30) + 3) is the constant 3 C4[4]).  Columns of `rest` above the active
 *  degree are not read.  One launch.
 *  gspl_sh_opacity_bwd: v_opacities [N] -> v_dc [N], v_rest [N, n_rest], EVERY element written (zeros in the columns above the active
 *  degree and in the rows the clamp cut): the gradient passes where 0 <= raw <= 1, both ends included as under torch.clamp, with raw
 *  recomputed from the inputs by the forward's own expression (nothing is saved).  A row whose incoming gradient is exactly zero is
 *  not evaluated and its coefficients are not read.  No gradient for means or origin (the reference detaches them).  One launch, no
 *  atomics: two runs give the same bits.
 * ---------------------------------------------------------------------------------------- */
int gspl_sh_opacity_fwd(int N, int degree, int n_rest, const float* means, const float* origin, const float* dc, const float* rest,
                        float* opacities, void* stream);
int gspl_sh_opacity_bwd(int N, int degree, int n_rest, const float* means, const float* origin, const float* dc, const float* rest,
                        const float* v_opacities, float* v_dc, float* v_rest, void* stream);

/* ------------------------------------------------------------------------------------------
 * 26. The per-frame front of the partition-LoD route (csrc/lod.hip).  PURELY ADDITIVE: two new entry points and three constants, no
 *    new struct, nothing existing changes, GSPL_ABI_VERSION stays 39.  What `PartitionLoDRendererModule.forward`
 *    (internal/renderers/partition_lod_renderer.py:550-625) does in front of the rasterizer: one level of detail per partition from the
 *    camera's distance, an optional frustum test, and the concatenation of the chosen models' property arrays.  The distance and the
 *    level rule are torch code there and are pinned directly (tests/lod_oracle.py against tests/golden/ref_lod.npz); the frustum test
 *    is pytorch3d's box overlap there and an exact separating-axis test here: parity with pytorch3d's build is UNPINNED, the two
 *    criteria differ for solids that touch.  fp32 data, device pointers only, no float atomics: two runs give the same bits.
 *
 *  The table: L levels x P partitions of Gaussians, every property one flat array over all segments; segment (level l, partition p)
 *  is rows seg_start[l P + p] .. seg_start[l P + p + 1] of each (seg_start [L P + 1] int64, rising).  1 <= P <= 65536, 1 <= L <= 127.
 *
 *  gspl_lod_select: ONE launch of one workgroup.  camera_center [3], transform [3, 3] (the orientation transform, row-major),
 *      box_min / box_max [P, 2], thresholds [L - 1] (NULL if and only if L == 1), prev_lod [P] int8 and prev_visible [P] u8 (the
 *      previous frame's; 127 in prev_lod marks "none yet").  Read with visibility_filter != 0 only (NULL allowed otherwise):
 *      boxes3d [P, 8, 3] world-space corners, one face clockwise and then the opposite face, corner i + 4 across an edge from
 *      corner i; world_to_camera [4, 4] as the reference keeps it (transposed: x_cam = x_world @ M[:3, :3] + M[3, :3]);
 *      K [3, 3] the intrinsics matrix; width, height.  Written:
 *      distance [P] = sqrt(sum(max(max(box_min - p, p - box_max), 0)^2)),  p = (camera_center @ transform)[:2], each operation rounded
 *        on its own, in the reference's order;
 *      lod [P] int8 = the smallest i with distance < thresholds[i], else L - 1;
 *      visible [P] u8 = 1 without the filter.  With it: the frustum has the image corners (0, 0), (W, 0), (W, H), (0, H) through
 *        K^-1 at depth 0.1 and at depth 10 max(distance); a partition is visible when NO axis among the 6 + 6 face normals (the cross
 *        product of a face's diagonals) and the 6 x 6 cross products of edge directions (two edges of the first face and the four
 *        edges between the faces, of either solid) separates its box, taken to camera space, from the frustum with a gap >= 0.  An
 *        axis a x b with |a x b|^2 <= 1e-12 |a|^2 |b|^2 is skipped.  The partition with the smallest distance (the lowest index
 *        among equals) is always visible.
 *      dst_start [P + 1] int64 = the exclusive scan of the chosen segments' lengths, an invisible partition counting 0 rows;
 *      record [2] int64 = { dst_start[P], changed }: changed = 1 when lod or visible differs from prev_lod / prev_visible anywhere.
 *      lod / visible may not alias prev_lod / prev_visible.
 *  gspl_lod_gather: ONE launch for the five arrays means [R, 3], shs [R, K, 3], opacities [R, 1], scales [R, 3], rotations [R, 4]
 *      (R = seg_start[L P], 1 <= K <= 64) -> the first n = dst_start[P] rows of out_*: rows dst_start[p] .. dst_start[p + 1] are the
 *      rows of segment (lod[p], p), in partition order.  Rows from n on are not touched.  All offsets are 64-bit (csrc/gspl_lod_index.h,
 *      built by the host compiler too).  A segment that does not lie inside 0 .. R, or a level outside 0 .. L - 1, copies nothing; no
 *      address outside the first n rows of an out_* array is ever written.  n == 0 succeeds without a launch.  Bit-exact copies.
 *  Anything else (P, L, K out of range, n > R, a NULL required pointer): GSPL_ERR_INVALID_ARG, nothing is launched.
 * ---------------------------------------------------------------------------------------- */
#define GSPL_LOD_MAX_PARTITIONS 65536
#define GSPL_LOD_MAX_LEVELS 127
#define GSPL_LOD_MAX_COEFFS 64
int gspl_lod_select(int P, int L, const float* camera_center, const float* transform, const float* box_min, const float* box_max,
                    const float* thresholds, const float* boxes3d, const float* world_to_camera, const float* K, int width, int height,
                    int visibility_filter, const int64_t* seg_start, const int8_t* prev_lod, const uint8_t* prev_visible,
                    float* distance, int8_t* lod, uint8_t* visible, int64_t* dst_start, int64_t* record, void* stream);
int gspl_lod_gather(int P, int L, int K, int64_t R, int64_t n, const int64_t* seg_start, const int8_t* lod, const int64_t* dst_start,
                    const float* means, const float* shs, const float* opacities, const float* scales, const float* rotations,
                    float* out_means, float* out_shs, float* out_opacities, float* out_scales, float* out_rotations, void* stream);

/* ------------------------------------------------------------------------------------------
 * 27. The scoring arithmetic of the Taming-3DGS density controller (csrc/taming.hip).  PURELY ADDITIVE: five new entry points and two
 *    constants, no new struct, nothing existing changes, GSPL_ABI_VERSION stays 39.  What `Taming3DGSUtils.normalize`, the aggregate of
 *    `compute_gaussian_score` and `get_edges` + the min-max normalisation of `on_train_start` compute
 *    (internal/density_controllers/taming_3dgs_density_controller.py:455-465, 536-553, 367-373, 138).  That arithmetic is torch code and
 *    one documented PIL filter, so it is pinned directly (tests/taming_oracle.py against tests/golden/ref_taming.npz).  Device pointers
 *    only, nothing is read by the host, no float atomics: two runs give the same bits.  Section 12's gspl_composite_scores supplies four
 *    of the rows.
 *
 *  Rows: `rows` is a HOST array of R device pointers (1 <= R <= 16), each to N entries of 4 bytes, 4-byte aligned; is_i32[r] != 0
 *  (host array too): the entries are int32 and stand for the value float(x).  An entry is VALID when its float32 bit pattern has the
 *  sign clear, is not zero and is at most 0x7f800000: > 0 and not NaN, +inf included, subnormals included whatever the flush mode.
 *  1 <= N <= 2^31 - 1; all indexing is 64-bit.  No row is written.
 *
 *  gspl_positive_medians: counts [R] int32 = the valid entries of each row, medians [R] = the valid entry of rank (counts - 1) / 2 in
 *      ascending order (torch.median's lower middle; NaN when counts is 0).  An exact radix select on the bit pattern: a memset of the
 *      counters, then three digit passes (11, 11 and 9 bits), each ONE launch over all rows (integer atomics into a histogram in LDS,
 *      flushed by integer atomics into the row's counters in the workspace, nonzero bins only) followed by ONE launch of a workgroup
 *      per row that scans the counters and fixes the digit holding the rank.  Plain launches in stream order; each pass reads every
 *      row once, front to back.  workspace: gspl_positive_medians_workspace_bytes(R) bytes (0 for an R out of range).
 *  gspl_taming_score_accumulate: ONE launch.  coeffs [R] (host), counts / medians [R] (device, of gspl_positive_medians on these rows),
 *      w [1] (device), visible [N] u8, importance [N] read and written:
 *          t_r = coeffs[r] * (v_r[g] / medians[r]) where v_r[g] is valid and counts[r] > 0, else 0          (quotient first, then c)
 *          a = (..(t_0 + t_1) + ..) + t_{n_first - 1},   b = (..(t_{n_first} + t_{n_first + 1}) + ..) + t_{R - 1}
 *          importance[g] = importance[g] + ((w * (b + a)) * (visible[g] ? 1 : 0))
 *      every operation rounded on its own (no contraction), in this association: the reference's, with the per-Gaussian rows first
 *      (1 <= n_first <= R; n_first == R: no second group).  As in the reference an invisible row whose sum is not finite becomes NaN.
 *      N == 0 succeeds without a launch.
 *  gspl_find_edges: image [3, H, W] uint8, or float32 in [0, 1] with is_float != 0, -> out [H, W] float32.  TWO launches.  A float is
 *      quantised as torchvision's ToPILImage does, x * 255 truncated (clamped to 0 .. 255, NaN to 0: undefined in the reference);
 *      grey = (R 19595 + G 38470 + B 7471 + 0x8000) >> 16 (PIL's L); e = 8 grey - the eight neighbours, clipped to 0 .. 255, in the
 *      interior, e = grey on the one-pixel border (PIL's FIND_EDGES); x = e / 255; out = (x - min x) / (max x - min x), each a float32
 *      operation.  A constant EDGE image (a black image, a constant one without an interior) gives 0 / 0 = NaN everywhere, as the reference does.  partial: n_partial >= gspl_find_edges_partials(H, W)
 *      pairs of int32 (the workgroups' smallest and largest e; 0 for a size out of range: H, W >= 1, H W <= 2^31 - 1).
 *  Anything else (R, n_first, N out of range, a NULL or misaligned pointer): GSPL_ERR_INVALID_ARG, nothing is launched; a workspace or
 *  partial array too small: GSPL_ERR_WORKSPACE.
 * ---------------------------------------------------------------------------------------- */
#define GSPL_TAMING_MAX_ROWS 16
#define GSPL_TAMING_MEDIAN_BINS 2048
size_t gspl_positive_medians_workspace_bytes(int R);
int gspl_positive_medians(int R, int64_t N, const void* const* rows, const int32_t* is_i32, int32_t* counts, float* medians,
                          void* workspace, size_t workspace_bytes, void* stream);
int gspl_taming_score_accumulate(int R, int n_first, int64_t N, const void* const* rows, const int32_t* is_i32, const float* coeffs,
                                 const int32_t* counts, const float* medians, const float* w, const uint8_t* visible,
                                 float* importance, void* stream);
int gspl_find_edges_partials(int H, int W);
int gspl_find_edges(int H, int W, const void* image, int is_float, float* out, int32_t* partial, int n_partial, void* stream);

/* ------------------------------------------------------------------------------------------
 * 28. The 3D half of Mip-Splatting (csrc/mip.hip).  PURELY ADDITIVE: three new entry points and five constants, no new struct, nothing
 *    existing changes, GSPL_ABI_VERSION stays 39.  What `MipSplattingUtils.compute_3d_filter`, `apply_3d_filter` and
 *    `apply_3d_filter_on_scales` compute (internal/models/mip_splatting.py:98-200).  That arithmetic is torch code, so it is pinned
 *    directly (tests/mip_oracle.py against tests/golden/ref_mip.npz).  fp32, device pointers only, nothing is read by the host, no float
 *    atomics: two runs give the same bits.  The 2D half (the dilation and the compensation) is section 2's projection.
 *
 *  gspl_mip_filter3d: means [N, 3], cameras [C, 16]: per row the world-to-camera rotation R (9, row-major), T (3), fx, fy, width,
 *      height.  A memset of the workspace and TWO launches.  Per Gaussian (one per lane) and camera (uniform across the wave: the
 *      table is read by uniform loads, never per lane), every operation rounded on its own, in the reference's order:
 *          p = R x + T (per component fmaf(R2, z, fmaf(R1, y, R0 * x)) + T);  valid_depth = p.z > 0.01;  z = max(p.z, 0.001)
 *          px = p.x / z * fx + width / 2,  py = p.y / z * fy + height / 2
 *          valid = valid_depth && px >= -0.15f * width && px <= width * 1.15f && py >= -0.15f * height && py <= 1.15f * height
 *          distance = min(distance, z) over the valid cameras, from 100000;  valid_any = some camera is valid
 *      The first launch also takes the maximum of `distance` over the rows with valid_any (a wave reduction, then ONE integer
 *      atomicMax per workgroup on the bit pattern: exact, the values are positive) and the largest positive fx (0 when there is none).
 *      The second writes filter_3d [N] = (valid_any ? distance : that maximum) / max fx * (float)0.4472135954999579, two operations.
 *      When NO row is valid in any camera the reference raises (max() of an empty tensor); here every row keeps 100000.
 *      distance [N] and valid_any [N] u8 are optional outputs (NULL: not written).  workspace: GSPL_MIP_WORKSPACE_BYTES, 4-byte aligned.
 *      1 <= N <= 2^31 - 1 and C >= 1, else GSPL_ERR_INVALID_ARG.
 *  gspl_mip_apply_fwd: ONE launch.  scales [N, 3], opacities [N] or NULL, filter_3d [N] -> scales_out [N, 3], opacities_out [N].
 *      s = RAW_SCALES ? exp(scales) : scales;  o = RAW_OPACITIES ? 1 / (1 + exp(-opacities)) : opacities;  f2 = filter_3d^2
 *          scales_out_i = sqrt(s_i^2 + f2);   r_i = s_i / scales_out_i;   coef = r_0 r_1 r_2
 *          opacities_out = o * coef with COMPENSATE, o without;  opacities NULL (COMPENSATE only): opacities_out = coef
 *      coef is the product of three ratios <= 1, NOT the reference's sqrt(prod s_i^2 / prod (s_i^2 + f2)), whose float32 numerator is
 *      subnormal or zero from scales of about 1e-7 on (its autograd then returns inf / NaN): equal to rounding elsewhere.  Where
 *      f2 == 0 the scales pass unchanged and coef is exactly 1.  opacities_out NULL: only the scales are written.
 *  gspl_mip_apply_bwd: ONE launch, recomputed from the forward's inputs.  v_scales_out [N, 3] and v_opacities_out [N] (either may be
 *      NULL: zero) -> v_scales [N, 3] and, with opacities, v_opacities [N] (NULL: not wanted), the gradients of the inputs AS GIVEN
 *      (raw or activated), every element written.  filter_3d gets none.
 *  N == 0 succeeds without a launch in the two apply calls.  Unknown flag bits, RAW_OPACITIES without opacities, an opacities_out
 *  with neither opacities nor COMPENSATE, a NULL required pointer: GSPL_ERR_INVALID_ARG, nothing is launched.
 * ---------------------------------------------------------------------------------------- */
#define GSPL_MIP_CAMERA_FLOATS 16
#define GSPL_MIP_WORKSPACE_BYTES 8
#define GSPL_MIP_RAW_SCALES 1
#define GSPL_MIP_RAW_OPACITIES 2
#define GSPL_MIP_COMPENSATE 4
int gspl_mip_filter3d(int64_t N, int C, const float* means, const float* cameras, float* filter_3d, float* distance, uint8_t* valid_any,
                      void* workspace, void* stream);
int gspl_mip_apply_fwd(int64_t N, int flags, const float* scales, const float* opacities, const float* filter_3d, float* scales_out,
                       float* opacities_out, void* stream);
int gspl_mip_apply_bwd(int64_t N, int flags, const float* scales, const float* opacities, const float* filter_3d,
                       const float* v_scales_out, const float* v_opacities_out, float* v_scales, float* v_opacities, void* stream);

/* ------------------------------------------------------------------------------------------
 * 29. The depth-regularisation loss (csrc/depthloss.hip).  PURELY ADDITIVE: three new entry points and six constants, no new struct,
 *    nothing existing changes, GSPL_ABI_VERSION stays 39.  fp32, device pointers only, nothing is read by the host.
 *
 *  The depth loss: what HasInverseDepthMetricsModule.get_inverse_depth_metric (internal/metrics/inverse_depth_metrics.py:70-104) and
 *  DepthMetricsModule.get_inverse_depth_metric (internal/metrics/depth_metrics.py:52-61) compute, every operation rounded on its own:
 *      NONE    p' = p                                          MEDIAN  p' = p / median   (median[0] on the device, or median_value)
 *      MINMAX  p' = (p - min p) / ((max p - min p) + 1e-8f)    MEAN    p' = p / mean(gt), g' = g / mean(gt)   (before the masks)
 *      then p' and g' are both multiplied by gt_mask and by pixel_mask where given ([H, W]; float32, or bytes with *_u8 != 0);
 *      out[0] = sum_p |g' - p'| / (H W)  (L1)  or  sum_p (g' - p')^2 / (H W)  (L2), over ALL H W elements.
 *  gspl_depth_loss_fwd: a 16-byte memset of the workspace's head and at most TWO launches: the min / max or sum reduction (MINMAX and
 *      MEAN only), then the elementwise pass; each leaves one partial per workgroup of 2048 elements, and the workgroup that arrives
 *      last adds all partials in index order (agent-scope atomics for the hand-off, no float atomics): two runs give the same bits.
 *      workspace: gspl_depth_loss_workspace_bytes(H, W) bytes, 16-byte aligned; it keeps min / max / mean for the backward.
 *  gspl_depth_loss_bwd: one launch.  v_pred [H, W] = -(sign(g' - p') or 2 (g' - p')) (d p' / d p) grad_out[0] / (H W), every element
 *      written, sign(0) = 0; grad_out on the device; `workspace` as the forward left it.  min, max, median, mean(gt) carry no gradient.
 *  1 <= H W <= 2^31, else GSPL_ERR_INVALID_ARG; another `kind` (the reference's l1+ssim) is GSPL_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------------------------- */
#define GSPL_DEPTH_LOSS_L1 0
#define GSPL_DEPTH_LOSS_L2 1
#define GSPL_DEPTH_NORM_NONE 0
#define GSPL_DEPTH_NORM_MINMAX 1
#define GSPL_DEPTH_NORM_MEDIAN 2
#define GSPL_DEPTH_NORM_MEAN 3
size_t gspl_depth_loss_workspace_bytes(int H, int W);
int gspl_depth_loss_fwd(int H, int W, int kind, int normalize, const float* pred, const float* gt,
                        const float* median, float median_value,
                        const void* gt_mask, int gt_mask_u8, const void* pixel_mask, int pixel_mask_u8,
                        void* workspace, size_t workspace_bytes, float* out, void* stream);
int gspl_depth_loss_bwd(int H, int W, int kind, int normalize, const float* pred, const float* gt,
                        const float* median, float median_value,
                        const void* gt_mask, int gt_mask_u8, const void* pixel_mask, int pixel_mask_u8,
                        const void* workspace, const float* grad_out, float* v_pred, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSPL_HIP_H */

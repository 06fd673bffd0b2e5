// normals.hip — normal maps from depth maps, the 2DGS maps and the surface regulariser sums (gfx950, wave64); include/gspl_hip.h section 15.
//
// The pseudo surface normal of 2DGS (Huang et al., "2D Gaussian Splatting for Geometrically Accurate Radiance Fields") and of gsplat's
// `utils.depth_to_normal`: back-project every pixel, q(y, x) = depth(y, x) A (x, y, 1)^T, and take the normalised cross product of the
// central differences, n = normalize((q(y+1, x) - q(y-1, x)) x (q(y, x+1) - q(y, x-1))), zero on the one-pixel border.
//   * depth_normal_fwd_kernel / depth_normal_bwd_kernel: the stencil on a plain depth map.  The backward is a GATHER: pixel p adds up what
//     the four centres (y +- 1, x), (y, x +- 1) that read q(p) contribute, recomputing their cross products from `depth` (a radius-2
//     diamond), in a fixed order: bit-reproducible, no atomics, no intermediate buffer.
//   * surfel_maps_fwd_kernel / surfel_maps_bwd_kernel: what the 2DGS renderer derives from the rasterizer's `allmap` [7, H, W] in one pass per
//     direction: the world-space normal, the blended surface depth and the alpha-weighted normal of that depth.
//   * reg_partials_kernel + reg_final_kernel / reg_bwd_kernel: mean(1 - a.b) and mean(dist) as a fixed two-level sum, and their gradients.
// Bandwidth-bound stencils: one lane per pixel, the 64 lanes of a wave along x (64 x 4 workgroups), planar outputs written plane by plane
// (every store instruction of a wave covers 256 contiguous bytes); the neighbour reads of a wave are the rows above and below, served by
// L1 / L2.  No LDS: profiles/normals_kernel_resources.txt.
#include <cfloat>
#include "gspl_device.h"
#include "gspl_host.h"
#include "gspl_reduce.h"

namespace gspl {
namespace {

constexpr int kTX = 64, kTY = 4;        // stencil workgroup: one wave per image row segment
constexpr int kT = 256;                 // threads per workgroup of the regulariser kernels
constexpr float kEps = 1e-12f;          // F.normalize's eps
// The regulariser's sums.  One thread adds at most kRegChain terms serially; a workgroup's 256 sums go through a 6-level butterfly and a
// 3-add chain over its four waves (kRegTree); the final workgroup does the same over the partials.  tests/test_normals_gpu.py mirrors
// these three numbers in its error bound.
constexpr int kRegChain = 64;
constexpr int kRegTree = 6 + 3;
constexpr int64_t kRegPerPartial = (int64_t)kT * kRegChain;
constexpr int64_t kRegMaxPixels = kRegPerPartial * kT * kRegChain;      // 2^28: the final chain stays within kRegChain too

struct Rays { float a[9]; };

__device__ inline Rays load_rays(const float* __restrict__ A) {
    Rays R;
#pragma unroll
    for (int i = 0; i < 9; ++i) R.a[i] = A[i];
    return R;
}

template <bool NORM>
__device__ inline void ray(const Rays& R, int x, int y, float r[3]) {
    const float fx = (float)x, fy = (float)y;
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = R.a[3 * c] * fx + R.a[3 * c + 1] * fy + R.a[3 * c + 2];
    if (NORM) {
        const float inv = 1.f / fmaxf(sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]), kEps);
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] *= inv;
    }
}

__device__ inline bool interior(int x, int y, int H, int W) { return x >= 1 && y >= 1 && x <= W - 2 && y <= H - 2; }

// torch.nan_to_num(v, 0, 0): NaN and +inf -> 0, -inf -> the lowest finite value
__device__ inline float nan0(float v) { return (v != v || v == INFINITY) ? 0.f : (v == -INFINITY ? -FLT_MAX : v); }
__device__ inline bool is_finite(float v) { return fabsf(v) <= FLT_MAX; }

struct PlainDepth {
    const float* __restrict__ d;
    __device__ float operator()(int64_t p) const { return d[p]; }
};

// surf_depth = (1 - rho) nan0(allmap0 / alpha) + rho nan0(allmap5); the blend in fp64 so that the fp32 quotient, rho and the result are
// the only roundings (3 U in all)
struct SurfDepth {
    const float* __restrict__ a;
    int64_t P;
    double w0, w1;
    __device__ float operator()(int64_t p) const {
        const float e = nan0(a[p] / a[P + p]), m = nan0(a[5 * P + p]);
        return (float)((double)e * w0 + (double)m * w1);
    }
};

// dx = q(y+1, x) - q(y-1, x), dy = q(y, x+1) - q(y, x-1) at an interior pixel
template <bool NORM, class D>
__device__ inline void differences(const D& depth, const Rays& R, int W, int x, int y, float dx[3], float dy[3]) {
    const int64_t p = (int64_t)y * W + x;
    const float dd = depth(p + W), du = depth(p - W), dr = depth(p + 1), dl = depth(p - 1);
    float rd[3], ru[3], rr[3], rl[3];
    ray<NORM>(R, x, y + 1, rd);
    ray<NORM>(R, x, y - 1, ru);
    ray<NORM>(R, x + 1, y, rr);
    ray<NORM>(R, x - 1, y, rl);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        dx[c] = dd * rd[c] - du * ru[c];
        dy[c] = dr * rr[c] - dl * rl[c];
    }
}

__device__ inline void cross3(const float a[3], const float b[3], float c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

template <bool NORM, class D>
__device__ inline void normal_at(const D& depth, const Rays& R, int W, int x, int y, float n[3]) {
    float dx[3], dy[3], c[3];
    differences<NORM>(depth, R, W, x, y, dx, dy);
    cross3(dx, dy, c);
    const float inv = 1.f / fmaxf(sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), kEps);
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = c[i] * inv;
}

// What centre (cx, cy) with upstream gradient v of its normal adds to the gradient of one of the four points it reads: `vertical` picks
// dx (else dy), the caller applies the sign (+ for the y+1 / x+1 point).  n = c / max(|c|, eps), c = dx x dy:
//   v_c = (v - n (n.v)) / |c| above eps, v / eps below (F.normalize keeps the constant denominator there);  v_dx = dy x v_c,  v_dy = v_c x dx.
template <bool NORM, class D>
__device__ inline void centre_gradient(const D& depth, const Rays& R, int W, int cx, int cy, const float v[3], bool vertical, float g[3]) {
    float dx[3], dy[3], c[3], vc[3];
    differences<NORM>(depth, R, W, cx, cy, dx, dy);
    cross3(dx, dy, c);
    const float len = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    if (len > kEps) {
        const float inv = 1.f / len;
        const float n[3] = {c[0] * inv, c[1] * inv, c[2] * inv};
        const float nv = n[0] * v[0] + n[1] * v[1] + n[2] * v[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) vc[i] = (v[i] - n[i] * nv) * inv;
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) vc[i] = v[i] * (1.f / kEps);
    }
    if (vertical) cross3(dy, vc, g);
    else cross3(vc, dx, g);
}

// upstream gradient of a normal map: HWC / CHW image, optionally times a per-pixel weight (the detached alpha of the 2DGS maps)
struct Upstream {
    const float* __restrict__ v;
    const float* __restrict__ weight;       // nullable
    int layout;
    int64_t P;
    __device__ void operator()(int64_t p, float out[3]) const {
        const float w = weight ? weight[p] : 1.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = w * (layout == GSPL_LAYOUT_HWC ? v[p * 3 + c] : v[(int64_t)c * P + p]);
    }
};

// d L / d depth(p): the four centres that read q(p), in the fixed order up, down, left, right; then the chain rule through q = depth r
template <bool NORM, class D>
__device__ inline float depth_gradient(const D& depth, const Rays& R, const Upstream& up, int H, int W, int x, int y) {
    float s[3] = {0.f, 0.f, 0.f};
    const int cxs[4] = {x, x, x - 1, x + 1}, cys[4] = {y - 1, y + 1, y, y};
    const float sign[4] = {1.f, -1.f, 1.f, -1.f};       // p is the centre's y+1, y-1, x+1, x-1 point
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!interior(cxs[k], cys[k], H, W)) continue;
        float v[3], g[3];
        up((int64_t)cys[k] * W + cxs[k], v);
        centre_gradient<NORM>(depth, R, W, cxs[k], cys[k], v, k < 2, g);
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += sign[k] * g[c];
    }
    float r[3];
    ray<NORM>(R, x, y, r);
    return r[0] * s[0] + r[1] * s[1] + r[2] * s[2];
}

// ---- depth to normal, generic ----------------------------------------------------------------------------------------------------------
template <bool NORM>
__global__ __launch_bounds__(kTX * kTY) void depth_normal_fwd_kernel(int H, int W, const float* __restrict__ depth, const float* __restrict__ rays,
                                                                     int layout, float* __restrict__ normal) {
    const int x = blockIdx.x * kTX + threadIdx.x, y = blockIdx.y * kTY + threadIdx.y;
    if (x >= W || y >= H) return;
    const int64_t P = (int64_t)H * W, p = (int64_t)y * W + x;
    float n[3] = {0.f, 0.f, 0.f};
    if (interior(x, y, H, W)) normal_at<NORM>(PlainDepth{depth}, load_rays(rays), W, x, y, n);
#pragma unroll
    for (int c = 0; c < 3; ++c) normal[layout == GSPL_LAYOUT_HWC ? p * 3 + c : (int64_t)c * P + p] = n[c];
}

template <bool NORM>
__global__ __launch_bounds__(kTX * kTY) void depth_normal_bwd_kernel(int H, int W, const float* __restrict__ depth, const float* __restrict__ rays,
                                                                     const float* __restrict__ v_normal, int layout, float* __restrict__ v_depth) {
    const int x = blockIdx.x * kTX + threadIdx.x, y = blockIdx.y * kTY + threadIdx.y;
    if (x >= W || y >= H) return;
    const Upstream up{v_normal, nullptr, layout, (int64_t)H * W};
    v_depth[(int64_t)y * W + x] = depth_gradient<NORM>(PlainDepth{depth}, load_rays(rays), up, H, W, x, y);
}

// ---- the 2DGS maps ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTX * kTY) void surfel_maps_fwd_kernel(int H, int W, const float* __restrict__ allmap, const float* __restrict__ normal_rot,
                                                                    const float* __restrict__ rays, float depth_ratio, float* __restrict__ rend_normal,
                                                                    float* __restrict__ surf_depth, float* __restrict__ surf_normal) {
    const int x = blockIdx.x * kTX + threadIdx.x, y = blockIdx.y * kTY + threadIdx.y;
    if (x >= W || y >= H) return;
    const int64_t P = (int64_t)H * W, p = (int64_t)y * W + x;
    const SurfDepth depth{allmap, P, 1.0 - (double)depth_ratio, (double)depth_ratio};
    const Rays M = load_rays(normal_rot);
    const float v0 = allmap[2 * P + p], v1 = allmap[3 * P + p], v2 = allmap[4 * P + p];
#pragma unroll
    for (int c = 0; c < 3; ++c) rend_normal[(int64_t)c * P + p] = M.a[3 * c] * v0 + M.a[3 * c + 1] * v1 + M.a[3 * c + 2] * v2;
    surf_depth[p] = depth(p);
    float n[3] = {0.f, 0.f, 0.f};
    if (interior(x, y, H, W)) normal_at<false>(depth, load_rays(rays), W, x, y, n);
    const float alpha = allmap[P + p];
#pragma unroll
    for (int c = 0; c < 3; ++c) surf_normal[(int64_t)c * P + p] = n[c] * alpha;
}

// v_allmap [7, H, W], every element written.  Planes 0 and 1 are 0 where allmap0 / alpha is not finite and plane 5 where allmap5 is not
// (nan_to_num passes no gradient there; torch's division backward then makes NaN of 0 / 0, which is not reproduced); plane 6 is 0.
__global__ __launch_bounds__(kTX * kTY) void surfel_maps_bwd_kernel(int H, int W, const float* __restrict__ allmap, const float* __restrict__ normal_rot,
                                                                    const float* __restrict__ rays, float depth_ratio,
                                                                    const float* __restrict__ v_rend_normal, const float* __restrict__ v_surf_depth,
                                                                    const float* __restrict__ v_surf_normal, float* __restrict__ v_allmap) {
    const int x = blockIdx.x * kTX + threadIdx.x, y = blockIdx.y * kTY + threadIdx.y;
    if (x >= W || y >= H) return;
    const int64_t P = (int64_t)H * W, p = (int64_t)y * W + x;
    const float rho = depth_ratio, w0 = (float)(1.0 - (double)depth_ratio);
    float vd = v_surf_depth ? v_surf_depth[p] : 0.f;
    if (v_surf_normal) {
        const SurfDepth depth{allmap, P, 1.0 - (double)depth_ratio, (double)depth_ratio};
        const Upstream up{v_surf_normal, allmap + P, GSPL_LAYOUT_CHW, P};
        vd += depth_gradient<false>(depth, load_rays(rays), up, H, W, x, y);
    }
    const float a0 = allmap[p], alpha = allmap[P + p], a5 = allmap[5 * P + p];
    const float e = a0 / alpha;
    const float g0 = is_finite(e) ? vd * w0 / alpha : 0.f;
    v_allmap[p] = g0;
    v_allmap[P + p] = is_finite(e) ? -g0 * e : 0.f;
    float g[3] = {0.f, 0.f, 0.f};
    if (v_rend_normal) {
        const Rays M = load_rays(normal_rot);
        const float u0 = v_rend_normal[p], u1 = v_rend_normal[P + p], u2 = v_rend_normal[2 * P + p];
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = M.a[c] * u0 + M.a[3 + c] * u1 + M.a[6 + c] * u2;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v_allmap[(2 + c) * P + p] = g[c];
    v_allmap[5 * P + p] = is_finite(a5) ? vd * rho : 0.f;
    v_allmap[6 * P + p] = 0.f;
}

// ---- the regulariser sums (block_sum of gspl_reduce.h: lanes by xor butterfly, then the four waves in order) ---------------------------
__global__ __launch_bounds__(kT) void reg_partials_kernel(int64_t P, const float* __restrict__ a, const float* __restrict__ b,
                                                          const float* __restrict__ dist, float* __restrict__ partials) {
    __shared__ float sh[kT / 64];
    const int64_t base = (int64_t)blockIdx.x * kRegPerPartial + threadIdx.x;
    float sn = 0.f, sd = 0.f;
    for (int k = 0; k < kRegChain; ++k) {
        const int64_t p = base + (int64_t)k * kT;
        if (p >= P) break;
        sn += 1.f - (a[p] * b[p] + a[P + p] * b[P + p] + a[2 * P + p] * b[2 * P + p]);
        if (dist) sd += dist[p];
    }
    const float tn = block_sum<kT>(sn, sh), td = block_sum<kT>(sd, sh);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = tn;
        partials[2 * blockIdx.x + 1] = td;
    }
}

__global__ __launch_bounds__(kT) void reg_final_kernel(int n_partials, float inv_p, const float* __restrict__ partials, float* __restrict__ out) {
    __shared__ float sh[kT / 64];
    float sn = 0.f, sd = 0.f;
    for (int j = threadIdx.x; j < n_partials; j += kT) {
        sn += partials[2 * j];
        sd += partials[2 * j + 1];
    }
    const float tn = block_sum<kT>(sn, sh), td = block_sum<kT>(sd, sh);
    if (threadIdx.x == 0) {
        out[0] = tn * inv_p;
        out[1] = td * inv_p;
    }
}

__global__ __launch_bounds__(kT) void reg_bwd_kernel(int64_t P, float inv_p, const float* __restrict__ a, const float* __restrict__ b,
                                                     const float* __restrict__ grad_out, float* __restrict__ v_a, float* __restrict__ v_b,
                                                     float* __restrict__ v_dist) {
    const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (p >= P) return;
    const float gn = -grad_out[0] * inv_p, gd = grad_out[1] * inv_p;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (v_a) v_a[(int64_t)c * P + p] = gn * b[(int64_t)c * P + p];
        if (v_b) v_b[(int64_t)c * P + p] = gn * a[(int64_t)c * P + p];
    }
    if (v_dist) v_dist[p] = gd;
}

inline bool shape_ok(int H, int W) { return H >= 0 && W >= 0 && ((int64_t)H + kTY - 1) / kTY <= 65535; }
inline dim3 stencil_grid(int H, int W) { return dim3((unsigned)((W + kTX - 1) / kTX), (unsigned)((H + kTY - 1) / kTY)); }
inline bool layout_ok(int layout) { return layout == GSPL_LAYOUT_HWC || layout == GSPL_LAYOUT_CHW; }

}  // namespace
}  // namespace gspl

extern "C" int gspl_depth_normal_fwd(int H, int W, const float* depth, const float* rays, int normalize_rays, int layout, float* normal,
                                     void* stream) {
    using namespace gspl;
    if (!shape_ok(H, W) || !layout_ok(layout)) return fail_arg("depth_normal_fwd: bad image shape (H <= 262140) or layout");
    if ((int64_t)H * W == 0) return GSPL_OK;
    if (!depth || !rays || !normal) return fail_arg("depth_normal_fwd: NULL pointer");
    const dim3 grid = stencil_grid(H, W), block(kTX, kTY);
    if (normalize_rays) hipLaunchKernelGGL(depth_normal_fwd_kernel<true>, grid, block, 0, (hipStream_t)stream, H, W, depth, rays, layout, normal);
    else hipLaunchKernelGGL(depth_normal_fwd_kernel<false>, grid, block, 0, (hipStream_t)stream, H, W, depth, rays, layout, normal);
    return check_launch("depth_normal_fwd");
}

extern "C" int gspl_depth_normal_bwd(int H, int W, const float* depth, const float* rays, int normalize_rays, const float* v_normal, int layout,
                                     float* v_depth, void* stream) {
    using namespace gspl;
    if (!shape_ok(H, W) || !layout_ok(layout)) return fail_arg("depth_normal_bwd: bad image shape (H <= 262140) or layout");
    if ((int64_t)H * W == 0) return GSPL_OK;
    if (!depth || !rays || !v_normal || !v_depth) return fail_arg("depth_normal_bwd: NULL pointer");
    const dim3 grid = stencil_grid(H, W), block(kTX, kTY);
    if (normalize_rays) hipLaunchKernelGGL(depth_normal_bwd_kernel<true>, grid, block, 0, (hipStream_t)stream, H, W, depth, rays, v_normal, layout, v_depth);
    else hipLaunchKernelGGL(depth_normal_bwd_kernel<false>, grid, block, 0, (hipStream_t)stream, H, W, depth, rays, v_normal, layout, v_depth);
    return check_launch("depth_normal_bwd");
}

extern "C" int gspl_surfel_maps_fwd(int H, int W, const float* allmap, const float* normal_rot, const float* rays, float depth_ratio,
                                    float* rend_normal, float* surf_depth, float* surf_normal, void* stream) {
    using namespace gspl;
    if (!shape_ok(H, W)) return fail_arg("surfel_maps_fwd: bad image shape (H <= 262140)");
    if ((int64_t)H * W == 0) return GSPL_OK;
    if (!allmap || !normal_rot || !rays || !rend_normal || !surf_depth || !surf_normal) return fail_arg("surfel_maps_fwd: NULL pointer");
    hipLaunchKernelGGL(surfel_maps_fwd_kernel, stencil_grid(H, W), dim3(kTX, kTY), 0, (hipStream_t)stream, H, W, allmap, normal_rot, rays,
                       depth_ratio, rend_normal, surf_depth, surf_normal);
    return check_launch("surfel_maps_fwd");
}

extern "C" int gspl_surfel_maps_bwd(int H, int W, const float* allmap, const float* normal_rot, const float* rays, float depth_ratio,
                                    const float* v_rend_normal, const float* v_surf_depth, const float* v_surf_normal, float* v_allmap,
                                    void* stream) {
    using namespace gspl;
    if (!shape_ok(H, W)) return fail_arg("surfel_maps_bwd: bad image shape (H <= 262140)");
    if ((int64_t)H * W == 0) return GSPL_OK;
    if (!allmap || !normal_rot || !rays || !v_allmap) return fail_arg("surfel_maps_bwd: NULL pointer");
    hipLaunchKernelGGL(surfel_maps_bwd_kernel, stencil_grid(H, W), dim3(kTX, kTY), 0, (hipStream_t)stream, H, W, allmap, normal_rot, rays,
                       depth_ratio, v_rend_normal, v_surf_depth, v_surf_normal, v_allmap);
    return check_launch("surfel_maps_bwd");
}

extern "C" int gspl_surface_reg_partials(int64_t n) {
    using namespace gspl;
    if (n <= 0) return 1;
    return (int)((n + kRegPerPartial - 1) / kRegPerPartial);
}

extern "C" int gspl_surface_reg_fwd(int H, int W, const float* a, const float* b, const float* dist, float* partials, float* out, void* stream) {
    using namespace gspl;
    const int64_t P = (int64_t)H * W;
    if (H < 1 || W < 1 || P > kRegMaxPixels) return fail_arg("surface_reg_fwd: 1 <= H W <= 2^28 (the mean of nothing is undefined)");
    if (!a || !b || !partials || !out) return fail_arg("surface_reg_fwd: NULL pointer");
    const int G = gspl_surface_reg_partials(P);
    hipLaunchKernelGGL(reg_partials_kernel, dim3(G), dim3(kT), 0, (hipStream_t)stream, P, a, b, dist, partials);
    const int rc = check_launch("surface_reg_fwd");
    if (rc != GSPL_OK) return rc;
    hipLaunchKernelGGL(reg_final_kernel, dim3(1), dim3(kT), 0, (hipStream_t)stream, G, (float)(1.0 / (double)P), partials, out);
    return check_launch("surface_reg_fwd");
}

extern "C" int gspl_surface_reg_bwd(int H, int W, const float* a, const float* b, const float* grad_out, float* v_a, float* v_b, float* v_dist,
                                    void* stream) {
    using namespace gspl;
    const int64_t P = (int64_t)H * W;
    if (H < 1 || W < 1 || P > kRegMaxPixels) return fail_arg("surface_reg_bwd: 1 <= H W <= 2^28");
    if (!a || !b || !grad_out) return fail_arg("surface_reg_bwd: NULL pointer");
    hipLaunchKernelGGL(reg_bwd_kernel, dim3((unsigned)((P + kT - 1) / kT)), dim3(kT), 0, (hipStream_t)stream, P, (float)(1.0 / (double)P), a, b,
                       grad_out, v_a, v_b, v_dist);
    return check_launch("surface_reg_bwd");
}

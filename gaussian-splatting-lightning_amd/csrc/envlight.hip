// envlight.hip — cube-map sampling and the sky blend of the PVG renderer (gfx950, wave64); include/gspl_hip.h section 17.
//
// A learnable sky is a cube map `base` [6, R, R, 3] sampled along every pixel's view direction with bilinear filtering that runs
// seamlessly over the cube's edges: the OpenGL cube-map rules, which nvdiffrast's texture(filter_mode='linear', boundary_mode='cube')
// publishes too.  Parity with nvdiffrast's own build is unpinned; the definition in the header and the fp64 restatement of it under
// tests/ are what this file is held to.
//   * cube_taps(): the ONE place that turns a direction into at most four (texel, weight) pairs; both kernel pairs use it, forward and
//     backward.
//   * cubemap_fwd_kernel / cubemap_bwd_kernel: explicit directions [M,3]; one lane per direction.  The backward scatters the texture
//     gradient with fp32 atomics (global_atomic_add_f32 under -munsafe-fp-atomics) into a buffer the caller has cleared.
//   * blend_fwd_kernel / blend_bwd_kernel: the renderer's path.  Per pixel the camera ray is formed from a device table (rotation and
//     intrinsics, never read back by the host), rotated to the world, swapped to the map's axes, sampled, and blended:
//     out = rgb + (1 - alpha) sky.  Neither the direction grid nor the sky image exists in memory; one lane per pixel, the 64 lanes of a
//     wave along x, planar images read and written plane by plane.
// No LDS.  Texel indices are clamped into the texture whatever the direction holds.
#include <cfloat>
#include "gspl_device.h"
#include "gspl_host.h"

namespace gspl {
namespace {

constexpr int kT = 256;
constexpr float kEps = 1e-12f;          // F.normalize's eps

struct Taps {
    int idx[4];          // float offset of the texel's first channel in base (0 for a tap that is not live)
    float w[4];
    unsigned live;       // bit k: tap k has a texel; 0: a degenerate direction (value 0, no gradient)
};

// (face, sc, tc, ma) of a point: the major axis is x if |x| >= |y| and |x| >= |z|, else y if |y| >= |z|, else z
__device__ inline int select_face(float x, float y, float z, float* sc, float* tc, float* ma) {
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    if (ax >= ay && ax >= az) {
        *ma = ax;
        *tc = -y;
        if (x >= 0.f) { *sc = -z; return 0; }
        *sc = z;
        return 1;
    }
    if (ay >= az) {
        *ma = ay;
        *sc = x;
        if (y >= 0.f) { *tc = z; return 2; }
        *tc = -z;
        return 3;
    }
    *ma = az;
    *tc = -y;
    if (z >= 0.f) { *sc = x; return 4; }
    *sc = -x;
    return 5;
}

// the point of face `face`'s (extended) plane at (u, v) in [-1, 1] units, its major coordinate of magnitude m: select_face's inverse
__device__ inline void face_point(int face, float u, float v, float m, float* x, float* y, float* z) {
    switch (face) {
        case 0: *x = m; *y = -v; *z = -u; break;
        case 1: *x = -m; *y = -v; *z = u; break;
        case 2: *x = u; *y = m; *z = v; break;
        case 3: *x = u; *y = -m; *z = -v; break;
        case 4: *x = u; *y = -v; *z = m; break;
        default: *x = -u; *y = -v; *z = -m; break;
    }
}

__device__ inline int clamp_texel(int v, int R) { return min(max(v, 0), R - 1); }

__device__ inline Taps cube_taps(float lx, float ly, float lz, int R) {
    Taps T;
    T.live = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) { T.idx[k] = 0; T.w[k] = 0.f; }
    const float norm1 = fabsf(lx) + fabsf(ly) + fabsf(lz);
    if (!(norm1 > 0.f) || !(fabsf(lx) <= FLT_MAX && fabsf(ly) <= FLT_MAX && fabsf(lz) <= FLT_MAX)) return T;      // zero, NaN or infinite
    float sc, tc, ma;
    const int face = select_face(lx, ly, lz, &sc, &tc, &ma);
    const float fR = (float)R;
    const float x = (sc / ma + 1.f) * 0.5f * fR - 0.5f, y = (tc / ma + 1.f) * 0.5f * fR - 0.5f;
    const float xf = floorf(x), yf = floorf(y);
    const float fx = x - xf, fy = y - yf;
    const int x0 = min(max((int)xf, -1), R - 1), y0 = min(max((int)yf, -1), R - 1);
    const float inv_r = 1.f / fR;
    float kept = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int xi = x0 + (k & 1), yi = y0 + (k >> 1);
        const float w = ((k & 1) ? fx : 1.f - fx) * ((k >> 1) ? fy : 1.f - fy);
        const bool out_x = xi < 0 || xi >= R, out_y = yi < 0 || yi >= R;
        if (out_x && out_y) continue;                      // a cube corner has no texel: dropped, the rest renormalised below
        int f = face, tx = xi, ty = yi;
        if (out_x || out_y) {
            // the texel centre on this face's extended plane, folded over the shared edge: the overflowing coordinate becomes +-1, the
            // former major coordinate 1 - 1/R; the face and the nearest texel are selected again from the folded point
            float u = (2.f * (float)xi + 1.f) * inv_r - 1.f, v = (2.f * (float)yi + 1.f) * inv_r - 1.f;
            if (out_x) u = xi < 0 ? -1.f : 1.f;
            else v = yi < 0 ? -1.f : 1.f;
            float px, py, pz, s2, t2, m2;
            face_point(face, u, v, 1.f - inv_r, &px, &py, &pz);
            f = select_face(px, py, pz, &s2, &t2, &m2);
            tx = clamp_texel((int)floorf((s2 / m2 + 1.f) * 0.5f * fR), R);
            ty = clamp_texel((int)floorf((t2 / m2 + 1.f) * 0.5f * fR), R);
        }
        T.idx[k] = ((f * R + ty) * R + tx) * 3;
        T.w[k] = w;
        T.live |= 1u << k;
        kept += w;
    }
    if (T.live != 0xFu) {          // (the dropped tap carries at most a quarter of the weight)
        const float inv = 1.f / kept;
#pragma unroll
        for (int k = 0; k < 4; ++k) T.w[k] *= inv;
    }
    return T;
}

__device__ inline void sample(const Taps& T, const float* __restrict__ base, float sky[3]) {
    sky[0] = sky[1] = sky[2] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!(T.live >> k & 1u)) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) sky[c] = fmaf(T.w[k], base[T.idx[k] + c], sky[c]);
    }
}

__device__ inline void scatter(const Taps& T, const float g[3], float* __restrict__ g_base) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!(T.live >> k & 1u) || T.w[k] == 0.f) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) atomicAdd(&g_base[T.idx[k] + c], T.w[k] * g[c]);
    }
}

// ---- explicit directions -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void cubemap_fwd_kernel(int64_t M, int R, const float* __restrict__ dirs, const float* __restrict__ base,
                                                         float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= M) return;
    const Taps T = cube_taps(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], R);
    float sky[3];
    sample(T, base, sky);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * i + c] = sky[c];
}

__global__ __launch_bounds__(kT) void cubemap_bwd_kernel(int64_t M, int R, const float* __restrict__ dirs, const float* __restrict__ v_out,
                                                         float* __restrict__ g_base) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= M) return;
    const Taps T = cube_taps(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], R);
    const float g[3] = {v_out[3 * i], v_out[3 * i + 1], v_out[3 * i + 2]};
    scatter(T, g, g_base);
}

// ---- the fused blend ---------------------------------------------------------------------------------------------------------------------
// table: the camera-to-world rotation [3,3] row-major, then fx, fy, cx, cy (13 floats).  The direction the sampler gets:
// d = normalize(((u - cx + ju) / fx, (v - cy + jv) / fy, 1)), w = rotation d, l = (w.x, w.z, -w.y).
__device__ inline void pixel_direction(const float* __restrict__ table, const float* __restrict__ jitter, int64_t P, int64_t p, int u, int v,
                                       float l[3]) {
    const float ju = jitter ? jitter[p] : 0.5f, jv = jitter ? jitter[P + p] : 0.5f;
    const float dx = ((float)u - table[11] + ju) / table[9], dy = ((float)v - table[12] + jv) / table[10];
    const float inv = 1.f / fmaxf(sqrtf(dx * dx + dy * dy + 1.f), kEps);
    const float d0 = dx * inv, d1 = dy * inv, d2 = inv;
    const float wx = table[0] * d0 + table[1] * d1 + table[2] * d2;
    const float wy = table[3] * d0 + table[4] * d1 + table[5] * d2;
    const float wz = table[6] * d0 + table[7] * d1 + table[8] * d2;
    l[0] = wx;
    l[1] = wz;
    l[2] = -wy;
}

__global__ __launch_bounds__(kT) void blend_fwd_kernel(int H, int W, int R, const float* __restrict__ table, const float* __restrict__ rgb,
                                                       const float* __restrict__ alpha, const float* __restrict__ base,
                                                       const float* __restrict__ jitter, float* __restrict__ out, float* __restrict__ dirs_out) {
    const int64_t P = (int64_t)H * W, p = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (p >= P) return;
    float l[3], sky[3];
    pixel_direction(table, jitter, P, p, (int)(p % W), (int)(p / W), l);
    sample(cube_taps(l[0], l[1], l[2], R), base, sky);
    const float T = 1.f - alpha[p];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c * P + p] = __fadd_rn(rgb[c * P + p], __fmul_rn(T, sky[c]));      // the two roundings of the unfused form
    if (dirs_out) {
#pragma unroll
        for (int c = 0; c < 3; ++c) dirs_out[3 * p + c] = l[c];
    }
}

// g_alpha [H,W] (nullable) = -sum_c v_out_c sky_c; g_base (nullable, cleared by the caller) += w (1 - alpha) v_out
__global__ __launch_bounds__(kT) void blend_bwd_kernel(int H, int W, int R, const float* __restrict__ table, const float* __restrict__ alpha,
                                                       const float* __restrict__ base, const float* __restrict__ jitter,
                                                       const float* __restrict__ v_out, float* __restrict__ g_alpha, float* __restrict__ g_base) {
    const int64_t P = (int64_t)H * W, p = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (p >= P) return;
    float l[3];
    pixel_direction(table, jitter, P, p, (int)(p % W), (int)(p / W), l);
    const Taps taps = cube_taps(l[0], l[1], l[2], R);
    const float g[3] = {v_out[p], v_out[P + p], v_out[2 * P + p]};
    if (g_alpha) {
        float sky[3];
        sample(taps, base, sky);
        g_alpha[p] = -(g[0] * sky[0] + g[1] * sky[1] + g[2] * sky[2]);
    }
    if (g_base) {
        const float T = 1.f - alpha[p];
        const float tg[3] = {T * g[0], T * g[1], T * g[2]};
        scatter(taps, tg, g_base);
    }
}

inline bool res_ok(int R) { return R >= 1 && R <= 8192; }          // 6 R R 3 floats stay below 2^31
inline unsigned blocks(int64_t n) { return (unsigned)((n + kT - 1) / kT); }
constexpr int64_t kMaxItems = (int64_t)1 << 31;                     // samples / pixels per call (3 n floats are indexed in 64 bits)

}  // namespace
}  // namespace gspl

extern "C" int gspl_cubemap_fwd(int64_t M, int R, const float* dirs, const float* base, float* out, void* stream) {
    using namespace gspl;
    if (M < 0 || M >= kMaxItems || !res_ok(R)) return fail_arg("cubemap_fwd: 0 <= M < 2^31 and 1 <= R <= 8192");
    if (M == 0) return GSPL_OK;
    if (!dirs || !base || !out) return fail_arg("cubemap_fwd: NULL pointer");
    hipLaunchKernelGGL(cubemap_fwd_kernel, dim3(blocks(M)), dim3(kT), 0, (hipStream_t)stream, M, R, dirs, base, out);
    return check_launch("cubemap_fwd");
}

extern "C" int gspl_cubemap_bwd(int64_t M, int R, const float* dirs, const float* v_out, float* g_base, void* stream) {
    using namespace gspl;
    if (M < 0 || M >= kMaxItems || !res_ok(R)) return fail_arg("cubemap_bwd: 0 <= M < 2^31 and 1 <= R <= 8192");
    if (M == 0) return GSPL_OK;
    if (!dirs || !v_out || !g_base) return fail_arg("cubemap_bwd: NULL pointer");
    hipLaunchKernelGGL(cubemap_bwd_kernel, dim3(blocks(M)), dim3(kT), 0, (hipStream_t)stream, M, R, dirs, v_out, g_base);
    return check_launch("cubemap_bwd");
}

extern "C" int gspl_envlight_blend_fwd(int H, int W, int R, const float* table, const float* rgb, const float* alpha, const float* base,
                                       const float* jitter, float* out, float* dirs_out, void* stream) {
    using namespace gspl;
    const int64_t P = (int64_t)H * W;
    if (H < 0 || W < 0 || P >= kMaxItems || !res_ok(R)) return fail_arg("envlight_blend_fwd: 0 <= H W < 2^31 and 1 <= R <= 8192");
    if (P == 0) return GSPL_OK;
    if (!table || !rgb || !alpha || !base || !out) return fail_arg("envlight_blend_fwd: NULL pointer");
    hipLaunchKernelGGL(blend_fwd_kernel, dim3(blocks(P)), dim3(kT), 0, (hipStream_t)stream, H, W, R, table, rgb, alpha, base, jitter, out, dirs_out);
    return check_launch("envlight_blend_fwd");
}

extern "C" int gspl_envlight_blend_bwd(int H, int W, int R, const float* table, const float* alpha, const float* base, const float* jitter,
                                       const float* v_out, float* g_alpha, float* g_base, void* stream) {
    using namespace gspl;
    const int64_t P = (int64_t)H * W;
    if (H < 0 || W < 0 || P >= kMaxItems || !res_ok(R)) return fail_arg("envlight_blend_bwd: 0 <= H W < 2^31 and 1 <= R <= 8192");
    if (P == 0 || (!g_alpha && !g_base)) return GSPL_OK;
    if (!table || !alpha || !base || !v_out) return fail_arg("envlight_blend_bwd: NULL pointer");
    hipLaunchKernelGGL(blend_bwd_kernel, dim3(blocks(P)), dim3(kT), 0, (hipStream_t)stream, H, W, R, table, alpha, base, jitter, v_out, g_alpha, g_base);
    return check_launch("envlight_blend_bwd");
}

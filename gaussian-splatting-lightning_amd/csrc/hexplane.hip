// hexplane.hip — the HexPlane / K-Planes field of the 4D-GS route, forward and backward (gfx950).
//
// What `HexPlaneField` of the reference computes (internal/model_components/gs4d_hexplane.py: six `F.grid_sample` calls per level, a
// product chain and a cat); the rules are those of include/gspl_hip.h section 22.  The planes live in ONE flat channel-last table,
// [texel][F] per plane, so a corner is one contiguous row of 4 F bytes.  The level / plane table (the four resolutions and the six
// first rows of each level) is computed by the caller on the host and travels BY VALUE in the kernel arguments: a level is one
// blockIdx.y, so every read of it is a scalar load with a wave-uniform index.
//
// Forward: F / 4 lanes per (point, level), one float4 per lane and corner (8 lanes cover a 128-byte row at F = 32); the product over
//   the six planes is lane-local; one float4 store.
// Backward, table: F lanes per (point, level), one float per lane, so that one wave-instruction adds 64 / F whole rows (two 128-byte
//   rows at F = 32, one 256-byte row at F = 64).  A (point, level) whose F values of v_out are all zero adds nothing and a wave of
//   such points returns before it reads x.
// Backward, x (optional): F / 4 lanes per point walk the levels, then sum their three partial sums with a fixed butterfly; no
//   atomics, the same bits on every run.
//
// The pixel coordinate of an axis is computed in float32 in the documented order with contraction switched off (hp_normalise,
// hp_pixel): the oracle takes the same cell for every input.
#include <cstdint>
#include "gspl_host.h"

namespace gspl {

static constexpr int HP_MAX_LEVELS = 8;
static constexpr int HP_BLOCK = 256;

struct HpTable {
    uint32_t res[HP_MAX_LEVELS][4];      // R_x, R_y, R_z, R_t of the level
    uint32_t first[HP_MAX_LEVELS][6];    // first row of each plane of the level
    float lo[3], scale[3];               // aabb[0] and float32(2 / (aabb[1] - aabb[0]))
};

// the planes in the order of itertools.combinations(range(4), 2): axis a runs along the width
__device__ constexpr int HP_A[6] = {0, 0, 0, 1, 1, 2};
__device__ constexpr int HP_B[6] = {1, 2, 3, 2, 3, 3};

// One axis of one point at one level: the two texel indices, the fraction, and whether the coordinate lies strictly inside
struct HpAxis {
    uint32_t i0, i1;
    float f;
    bool has1;       // i0 + 1 is a texel (false only on the last texel, where f == 0)
    bool inside;     // 0 < i < R - 1 before the clamp: where grid_sample lets a gradient through
};

// The two steps of a pixel coordinate, every operation rounded on its own: the compiler's default would contract a product and the
// sum behind it into one fma (the __f*_rn intrinsics are plain operators to it), and the cell would differ from the reference's
__device__ __forceinline__ float hp_normalise(float x, float lo, float scale) {
#pragma clang fp contract(off)
    const float moved = x - lo;
    const float scaled = moved * scale;
    return scaled - 1.f;
}
__device__ __forceinline__ float hp_pixel(float c, float last) {
#pragma clang fp contract(off)
    const float shifted = c + 1.f;
    const float half = shifted * 0.5f;
    return half * last;
}

__device__ __forceinline__ HpAxis hp_axis(float c, uint32_t R) {
    const float last = (float)(R - 1);
    const float raw = hp_pixel(c, last);
    const float i = fminf(fmaxf(raw, 0.f), last);          // (a NaN becomes 0)
    const float fl = floorf(i);
    HpAxis a;
    a.i0 = min((uint32_t)fl, R - 1);
    a.has1 = a.i0 + 1 < R;
    a.i1 = a.has1 ? a.i0 + 1 : a.i0;
    a.f = i - fl;
    a.inside = raw > 0.f && raw < last;
    return a;
}

// p = (x_n, y_n, z_n, t) of point n, then the four axes at level l
__device__ __forceinline__ void hp_axes(const HpTable& tb, int l, const float* __restrict__ x, const float* __restrict__ t, float t_uniform,
                                        size_t n, HpAxis ax[4]) {
#pragma unroll
    for (int d = 0; d < 3; ++d)
        ax[d] = hp_axis(hp_normalise(x[n * 3 + d], tb.lo[d], tb.scale[d]), tb.res[l][d]);
    ax[3] = hp_axis(t ? t[n] : t_uniform, tb.res[l][3]);
}

// rows of the four corners of plane p, (a0 b0), (a1 b0), (a0 b1), (a1 b1), and their weights
struct HpCorners {
    uint32_t row[4];
    float w[4];
    bool live[4];
};

__device__ __forceinline__ HpCorners hp_corners(const HpTable& tb, int l, int p, const HpAxis ax[4]) {
    const HpAxis& a = ax[HP_A[p]];
    const HpAxis& b = ax[HP_B[p]];
    const uint32_t Ra = tb.res[l][HP_A[p]], first = tb.first[l][p];
    const float wa0 = 1.f - a.f, wb0 = 1.f - b.f;
    HpCorners c;
    c.row[0] = first + b.i0 * Ra + a.i0; c.w[0] = wa0 * wb0; c.live[0] = true;
    c.row[1] = first + b.i0 * Ra + a.i1; c.w[1] = a.f * wb0; c.live[1] = a.has1;
    c.row[2] = first + b.i1 * Ra + a.i0; c.w[2] = wa0 * b.f; c.live[2] = b.has1;
    c.row[3] = first + b.i1 * Ra + a.i1; c.w[3] = a.f * b.f; c.live[3] = a.has1 && b.has1;
    return c;
}

__device__ __forceinline__ float4 hp_mul(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 hp_fma(float w, float4 v, float4 acc) {
    return make_float4(fmaf(w, v.x, acc.x), fmaf(w, v.y, acc.y), fmaf(w, v.z, acc.z), fmaf(w, v.w, acc.w));
}
__device__ __forceinline__ float4 hp_scale(float w, float4 v) { return make_float4(w * v.x, w * v.y, w * v.z, w * v.w); }
__device__ __forceinline__ float4 hp_sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float hp_dot(float4 a, float4 b, float acc) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc)))); }

// the four corner values of a plane for this lane's four channels; a corner that is no texel reads as zero
template <int F>
__device__ __forceinline__ void hp_load4(const float* __restrict__ table, const HpCorners& c, int sub, float4 v[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = reinterpret_cast<const float4*>(table + (size_t)c.row[k] * F)[sub];
        if (!c.live[k]) v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

__device__ __forceinline__ float4 hp_interp(const HpCorners& c, const float4 v[4]) {
    return hp_fma(c.w[3], v[3], hp_fma(c.w[2], v[2], hp_fma(c.w[1], v[1], hp_scale(c.w[0], v[0]))));
}

template <int F>
__global__ __launch_bounds__(HP_BLOCK) void hexplane_fwd_kernel(int N, int L, HpTable tb, const float* __restrict__ x, const float* __restrict__ t,
                                                                float t_uniform, const float* __restrict__ table, float* __restrict__ out) {
    constexpr int LPP = F / 4;                     // lanes of a point
    const int l = blockIdx.y;
    const int sub = threadIdx.x % LPP;
    const size_t n = (size_t)blockIdx.x * (HP_BLOCK / LPP) + threadIdx.x / LPP;
    if (n >= (size_t)N) return;
    HpAxis ax[4];
    hp_axes(tb, l, x, t, t_uniform, n, ax);
    float4 acc;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        const HpCorners c = hp_corners(tb, l, p, ax);
        float4 v[4];
        hp_load4<F>(table, c, sub, v);
        const float4 i = hp_interp(c, v);
        acc = p == 0 ? i : hp_mul(acc, i);
    }
    reinterpret_cast<float4*>(out + (n * L + l) * F)[sub] = acc;
}

template <int F>
__global__ __launch_bounds__(HP_BLOCK) void hexplane_bwd_table_kernel(int N, int L, HpTable tb, const float* __restrict__ x, const float* __restrict__ t,
                                                                      float t_uniform, const float* __restrict__ table,
                                                                      const float* __restrict__ v_out, float* __restrict__ v_table) {
    const int l = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int f = threadIdx.x % F;
    const size_t n = (size_t)blockIdx.x * (HP_BLOCK / F) + threadIdx.x / F;
    const bool valid = n < (size_t)N;
    const float g = valid ? v_out[(n * L + l) * F + f] : 0.f;
    // a point takes part when one of its F values is not zero
    const unsigned long long nonzero = __ballot(g != 0.f);
    if (nonzero == 0) return;                      // the whole wave
    const unsigned long long group = F == 64 ? ~0ull : (((1ull << (F & 63)) - 1) << (lane & ~(F - 1)));
    if ((nonzero & group) == 0) return;
    HpAxis ax[4];
    hp_axes(tb, l, x, t, t_uniform, n, ax);
    HpCorners c[6];
    float interp[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        c[p] = hp_corners(tb, l, p, ax);
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v = c[p].live[k] ? table[(size_t)c[p].row[k] * F + f] : 0.f;
            acc = k == 0 ? c[p].w[0] * v : fmaf(c[p].w[k], v, acc);
        }
        interp[p] = acc;
    }
    // the product of the OTHER five planes, without a division: before[p] = I_0 .. I_{p-1}, after = I_{p+1} .. I_5
    float before[6], after = 1.f;
    before[0] = 1.f;
#pragma unroll
    for (int p = 1; p < 6; ++p) before[p] = before[p - 1] * interp[p - 1];
#pragma unroll
    for (int p = 5; p >= 0; --p) {
        const float go = g * (before[p] * after);
        after *= interp[p];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c[p].live[k]) atomicAdd(v_table + (size_t)c[p].row[k] * F + f, c[p].w[k] * go);
    }
}

template <int F>
__global__ __launch_bounds__(HP_BLOCK) void hexplane_bwd_x_kernel(int N, int L, HpTable tb, const float* __restrict__ x, const float* __restrict__ t,
                                                                  float t_uniform, const float* __restrict__ table,
                                                                  const float* __restrict__ v_out, float* __restrict__ v_x) {
    constexpr int LPP = F / 4;
    const int sub = threadIdx.x % LPP;
    const size_t n = (size_t)blockIdx.x * (HP_BLOCK / LPP) + threadIdx.x / LPP;
    const bool valid = n < (size_t)N;
    const size_t at = valid ? n : 0;               // every lane stays for the butterfly; N >= 1
    float acc[3] = {0.f, 0.f, 0.f};
    for (int l = 0; l < L; ++l) {
        const float4 g = reinterpret_cast<const float4*>(v_out + (at * L + l) * F)[sub];
        HpAxis ax[4];
        hp_axes(tb, l, x, t, t_uniform, at, ax);
        float4 interp[6], da[6], db[6];            // the plane's value and its derivatives along its two pixel axes
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            const HpCorners c = hp_corners(tb, l, p, ax);
            float4 v[4];
            hp_load4<F>(table, c, sub, v);
            interp[p] = hp_interp(c, v);
            const float fa = ax[HP_A[p]].f, fb = ax[HP_B[p]].f;
            da[p] = hp_fma(fb, hp_sub(v[3], v[2]), hp_scale(1.f - fb, hp_sub(v[1], v[0])));
            db[p] = hp_fma(fa, hp_sub(v[3], v[1]), hp_scale(1.f - fa, hp_sub(v[2], v[0])));
        }
        float4 before[6], after = make_float4(1.f, 1.f, 1.f, 1.f);
        before[0] = after;
#pragma unroll
        for (int p = 1; p < 6; ++p) before[p] = hp_mul(before[p - 1], interp[p - 1]);
        float level[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int p = 5; p >= 0; --p) {
            const float4 go = hp_mul(g, hp_mul(before[p], after));
            after = hp_mul(after, interp[p]);
            level[HP_A[p]] = hp_dot(da[p], go, level[HP_A[p]]);          // (axis a of a plane is never the time)
            if (HP_B[p] < 3) level[HP_B[p]] = hp_dot(db[p], go, level[HP_B[p]]);
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float pixels = ax[d].inside ? ((float)(tb.res[l][d] - 1) * 0.5f) * tb.scale[d] : 0.f;
            acc[d] = fmaf(pixels, level[d], acc[d]);
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
#pragma unroll
        for (int m = 1; m < LPP; m *= 2) acc[d] += __shfl_xor(acc[d], m, 64);
    }
    if (valid && sub == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) v_x[n * 3 + d] = acc[d];
    }
}

// The argument checks both entries share; fills `tb`.  resolutions [L, 4], offsets [6 L + 1] and box [6] are HOST arrays.  A plane's
// rows must be exactly R_a R_b, so no clamped index can address outside the table.
static int hp_table(const char* who, int N, int F, int L, const uint32_t* resolutions, const uint32_t* offsets, const float* box, HpTable& tb) {
    if (N < 0) return fail_arg(who);
    if (F != 8 && F != 16 && F != 32 && F != 64) { set_error(who, "F (features per plane) must be 8, 16, 32 or 64"); return GSPL_ERR_INVALID_ARG; }
    if (L < 1 || L > HP_MAX_LEVELS) { set_error(who, "L (levels) must be 1 .. 8"); return GSPL_ERR_INVALID_ARG; }
    if (!resolutions || !offsets || !box) return fail_arg(who);
    if (offsets[6 * L] > 0x7fffffffu) { set_error(who, "the table has at most 2^31 - 1 rows"); return GSPL_ERR_INVALID_ARG; }
    for (int l = 0; l < HP_MAX_LEVELS; ++l) {
        for (int d = 0; d < 4; ++d) {
            tb.res[l][d] = l < L ? resolutions[4 * l + d] : 1;
            if (tb.res[l][d] < 1 || tb.res[l][d] > (1u << 15)) { set_error(who, "every resolution must be 1 .. 32768"); return GSPL_ERR_INVALID_ARG; }
        }
        constexpr int A[6] = {0, 0, 0, 1, 1, 2}, B[6] = {1, 2, 3, 2, 3, 3};
        for (int p = 0; p < 6; ++p) {
            tb.first[l][p] = l < L ? offsets[6 * l + p] : 0;
            if (l < L && (offsets[6 * l + p + 1] < offsets[6 * l + p] || offsets[6 * l + p + 1] - offsets[6 * l + p] != tb.res[l][A[p]] * tb.res[l][B[p]])) {
                set_error(who, "offsets must give every plane exactly R_a R_b rows");
                return GSPL_ERR_INVALID_ARG;
            }
        }
    }
    for (int d = 0; d < 3; ++d) { tb.lo[d] = box[d]; tb.scale[d] = box[3 + d]; }
    return GSPL_OK;
}

}  // namespace gspl

using namespace gspl;

extern "C" int gspl_hexplane_fwd(int N, int F, int L, const uint32_t* resolutions, const uint32_t* offsets, const float* box,
                                 const float* x, const float* t, float t_uniform, const float* table, float* out, void* stream) {
    HpTable tb;
    if (const int rc = hp_table("gspl_hexplane_fwd", N, F, L, resolutions, offsets, box, tb)) return rc;
    if (N == 0) return GSPL_OK;
    if (!x || !table || !out) return fail_arg("gspl_hexplane_fwd");
    if (!aligned16(table) || !aligned16(out)) { set_error("gspl_hexplane_fwd", "table and out must be aligned to 16 bytes"); return GSPL_ERR_INVALID_ARG; }
    return dispatch_int<8, 16, 32, 64>(F, [&](auto f) {      // (hp_table has refused every other F)
        constexpr int points = HP_BLOCK / (decltype(f)::value / 4);
        hipLaunchKernelGGL((hexplane_fwd_kernel<decltype(f)::value>), dim3((N + points - 1) / points, L), dim3(HP_BLOCK), 0, (hipStream_t)stream,
                           N, L, tb, x, t, t_uniform, table, out);
        return check_launch("gspl_hexplane_fwd");
    });
}

extern "C" int gspl_hexplane_bwd(int N, int F, int L, const uint32_t* resolutions, const uint32_t* offsets, const float* box,
                                 const float* x, const float* t, float t_uniform, const float* table, const float* v_out,
                                 float* v_table, float* v_x, void* stream) {
    HpTable tb;
    if (const int rc = hp_table("gspl_hexplane_bwd", N, F, L, resolutions, offsets, box, tb)) return rc;
    if (N == 0) return GSPL_OK;
    if (!x || !table || !v_out || (!v_table && !v_x)) return fail_arg("gspl_hexplane_bwd");
    if (!aligned16(table) || !aligned16(v_out)) { set_error("gspl_hexplane_bwd", "table and v_out must be aligned to 16 bytes"); return GSPL_ERR_INVALID_ARG; }
    return dispatch_int<8, 16, 32, 64>(F, [&](auto f) {      // (hp_table has refused every other F)
        if (v_table) {
            constexpr int points = HP_BLOCK / decltype(f)::value;
            hipLaunchKernelGGL((hexplane_bwd_table_kernel<decltype(f)::value>), dim3((N + points - 1) / points, L), dim3(HP_BLOCK), 0, (hipStream_t)stream,
                               N, L, tb, x, t, t_uniform, table, v_out, v_table);
            if (const int rc = check_launch("gspl_hexplane_bwd (table)")) return rc;
        }
        if (v_x) {
            constexpr int points = HP_BLOCK / (decltype(f)::value / 4);
            hipLaunchKernelGGL((hexplane_bwd_x_kernel<decltype(f)::value>), dim3((N + points - 1) / points), dim3(HP_BLOCK), 0, (hipStream_t)stream,
                               N, L, tb, x, t, t_uniform, table, v_out, v_x);
            return check_launch("gspl_hexplane_bwd (x)");
        }
        return (int)GSPL_OK;
    });
}

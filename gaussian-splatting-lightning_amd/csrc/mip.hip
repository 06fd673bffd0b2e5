// mip.hip — the 3D half of the Mip-Splatting route: the 3D filter of every Gaussian over all training cameras, and its application
// to scales and opacities, forward and backward (gfx950; include/gspl_hip.h section 28).
//
// Restates internal/models/mip_splatting.py `MipSplattingUtils.compute_3d_filter` (:98-162), `apply_3d_filter_on_scales` (:165-180)
// and `apply_3d_filter` (:183-200).  The reference's arithmetic is torch code: tests/mip_oracle.py (fp64) is pinned to it through
// tests/golden/ref_mip.npz, and these kernels to the oracle.
//
// Filter: one Gaussian per lane, the camera loop inside the lane.  The camera index is the same in all 64 lanes and the table is a
// read-only kernel argument, so a camera's 16 floats arrive through uniform (scalar) loads into SGPRs: 64 bytes per camera and WAVE,
// nothing per lane, no LDS.  Per Gaussian and camera about 40 VALU instructions (two correctly rounded divisions are most of them);
// 12 bytes read and 4 .. 9 written per Gaussian: compute-bound from a few cameras on.  The reference's operations are rounded one by
// one (no contraction): only p = R x + T is an explicit fmaf chain, which the reference's matmul does not pin either.
//
// Apply: HBM-bound, 16 (20) bytes read and 12 (16) written per row forward.  Lane-per-row reads of the 12-byte scale rows: the three
// loads of a wave cover the same 768 contiguous bytes, every cache line is used in full.
//
// The opacity coefficient is the PRODUCT OF THE THREE RATIOS r_i = s_i / sqrt(s_i^2 + f^2), each at most 1, never
// sqrt(prod s_i^2 / prod (s_i^2 + f^2)) as the reference writes it: in float32 prod s_i^2 is subnormal or zero from scales of about
// 1e-7 on, where the reference's quotient loses all digits and its autograd returns inf / NaN.  The two forms agree to rounding
// wherever the reference's is normal.  Where f^2 == 0 the filter is absent: the scales pass unchanged and the coefficient is exactly 1.
//
// No float atomics, no scratch, nothing read by the host: two runs give the same bits.
#pragma clang fp contract(off)
#include "gspl_device.h"
#include "gspl_host.h"

namespace gspl {

static constexpr int MIP_BLOCK = 256;
static constexpr float MIP_FAR = 100000.0f;                     // the reference's initial distance
static constexpr float MIP_SQRT_0_2 = 0.4472135954999579f;      // (float)(0.2 ** 0.5)

__device__ __forceinline__ float wave_max_nonneg(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// stats[0]: the bit pattern of the largest distance of a row valid in some camera (0: there is none); stats[1]: of the largest fx
// (0: none is positive, the reference's `focal_length = 0.`).  Both are floats >= 0, for which the integer order is the float order.
// `filter` receives the row's distance, or -1 where no camera sees it: the second launch reads it back in place.
__global__ __launch_bounds__(MIP_BLOCK) void mip_filter3d_distance_kernel(
    int64_t N, int C, const float* __restrict__ means, const float* __restrict__ cams, float* __restrict__ filter,
    float* __restrict__ distance, uint8_t* __restrict__ valid_any, int* __restrict__ stats) {
    __shared__ float wave_max[MIP_BLOCK / 64];
    const int64_t n = (int64_t)blockIdx.x * MIP_BLOCK + threadIdx.x;
    const bool live = n < N;
    const int64_t m = live ? n : N - 1;
    const float x = means[m * 3 + 0], y = means[m * 3 + 1], z = means[m * 3 + 2];
    float dist = MIP_FAR, max_fx = 0.f;
    bool any = false;
    for (int c = 0; c < C; ++c) {
        const float* __restrict__ k = cams + (size_t)c * GSPL_MIP_CAMERA_FLOATS;      // uniform: R [9] row-major, T [3], fx, fy, width, height
        const float fx = k[12], fy = k[13], w = k[14], h = k[15];
        const float px0 = fmaf(k[2], z, fmaf(k[1], y, k[0] * x)) + k[9];
        const float py0 = fmaf(k[5], z, fmaf(k[4], y, k[3] * x)) + k[10];
        const float pz0 = fmaf(k[8], z, fmaf(k[7], y, k[6] * x)) + k[11];
        const bool valid_depth = pz0 > 0.01f;
        const float pz = fmaxf(pz0, 0.001f);
        const float px = px0 / pz * fx + w / 2.0f;
        const float py = py0 / pz * fy + h / 2.0f;
        const bool in_screen = (px >= -0.15f * w) && (px <= w * 1.15f) && (py >= -0.15f * h) && (py <= 1.15f * h);
        const bool valid = valid_depth && in_screen;
        dist = valid ? fminf(dist, pz) : dist;
        any = any || valid;
        max_fx = fx > max_fx ? fx : max_fx;
    }
    if (live) {
        filter[n] = any ? dist : -1.f;
        if (distance) distance[n] = dist;
        if (valid_any) valid_any[n] = any ? 1 : 0;
    }
    const float mine = wave_max_nonneg(live && any ? dist : 0.f);
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        float b = wave_max[0];
#pragma unroll
        for (int wv = 1; wv < MIP_BLOCK / 64; ++wv) b = fmaxf(b, wave_max[wv]);
        if (b > 0.f) atomicMax(&stats[0], __float_as_int(b));
        if (blockIdx.x == 0) stats[1] = __float_as_int(max_fx);
    }
}

// filter_3d = (valid ? distance : the largest valid distance) / max fx * sqrt(0.2): two operations, each rounded
__global__ __launch_bounds__(MIP_BLOCK) void mip_filter3d_finish_kernel(int64_t N, float* __restrict__ filter, const int* __restrict__ stats) {
    const int64_t n = (int64_t)blockIdx.x * MIP_BLOCK + threadIdx.x;
    if (n >= N) return;
    const int bits = stats[0];
    const float fill = bits ? __int_as_float(bits) : MIP_FAR;      // no row valid anywhere: every row keeps the initial distance
    const float max_fx = __int_as_float(stats[1]);
    const float d0 = filter[n];
    const float d = d0 < 0.f ? fill : d0;
    filter[n] = d / max_fx * MIP_SQRT_0_2;
}

// ---- apply ----------------------------------------------------------------------------------------------------------------------------
struct MipRow {
    float s[3];       // activated scales
    float out[3];     // sqrt(s^2 + f^2)
    float b[3];       // s^2 + f^2
    float r[3];       // s / out
    float f2;
    bool plain;       // f^2 == 0: no filter
};

template <bool RAW_S>
__device__ __forceinline__ MipRow mip_row(const float* __restrict__ scales, const float* __restrict__ filter_3d, int64_t n) {
    MipRow q;
    const float f = filter_3d[n];
    q.f2 = f * f;
    q.plain = q.f2 == 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float v = scales[n * 3 + i];
        q.s[i] = RAW_S ? expf(v) : v;
        q.b[i] = q.s[i] * q.s[i] + q.f2;
        q.out[i] = q.plain ? q.s[i] : sqrtf(q.b[i]);
        q.r[i] = q.plain ? 1.f : q.s[i] / q.out[i];
    }
    return q;
}

template <bool RAW_O>
__device__ __forceinline__ float mip_opacity(float v) { return RAW_O ? 1.f / (1.f + expf(-v)) : v; }

template <bool RAW_S, bool RAW_O, bool COMP>
__global__ __launch_bounds__(MIP_BLOCK) void mip_apply_fwd_kernel(int64_t N, const float* __restrict__ scales, const float* __restrict__ opacities,
                                                                  const float* __restrict__ filter_3d, float* __restrict__ scales_out,
                                                                  float* __restrict__ opacities_out) {
    const int64_t n = (int64_t)blockIdx.x * MIP_BLOCK + threadIdx.x;
    if (n >= N) return;
    const MipRow q = mip_row<RAW_S>(scales, filter_3d, n);
#pragma unroll
    for (int i = 0; i < 3; ++i) scales_out[n * 3 + i] = q.out[i];
    if (!opacities_out) return;
    const float coef = q.r[0] * q.r[1] * q.r[2];
    if (opacities) {
        const float o = mip_opacity<RAW_O>(opacities[n]);
        opacities_out[n] = COMP ? o * coef : o;
    } else {
        opacities_out[n] = coef;
    }
}

// d out_i / d s_i = r_i;  d r_i / d s_i = f^2 / (out_i b_i);  coef = r_0 r_1 r_2;  raw inputs: d s / d raw = s, d o / d raw = o (1 - o)
template <bool RAW_S, bool RAW_O, bool COMP>
__global__ __launch_bounds__(MIP_BLOCK) void mip_apply_bwd_kernel(int64_t N, const float* __restrict__ scales, const float* __restrict__ opacities,
                                                                  const float* __restrict__ filter_3d, const float* __restrict__ v_scales_out,
                                                                  const float* __restrict__ v_opacities_out, float* __restrict__ v_scales,
                                                                  float* __restrict__ v_opacities) {
    const int64_t n = (int64_t)blockIdx.x * MIP_BLOCK + threadIdx.x;
    if (n >= N) return;
    const MipRow q = mip_row<RAW_S>(scales, filter_3d, n);
    const float v_o = v_opacities_out ? v_opacities_out[n] : 0.f;
    const float coef = q.r[0] * q.r[1] * q.r[2];
    float v_coef = 0.f;
    if (opacities) {
        const float o = mip_opacity<RAW_O>(opacities[n]);
        if (COMP) v_coef = v_o * o;
        if (v_opacities) {
            const float g = COMP ? v_o * coef : v_o;
            v_opacities[n] = RAW_O ? g * (o * (1.f - o)) : g;
        }
    } else {
        v_coef = v_o;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float others = q.r[(i + 1) % 3] * q.r[(i + 2) % 3];
        const float dr = q.plain ? 0.f : q.f2 / (q.out[i] * q.b[i]);
        const float v_out = v_scales_out ? v_scales_out[n * 3 + i] : 0.f;
        const float g = v_out * q.r[i] + v_coef * others * dr;
        v_scales[n * 3 + i] = RAW_S ? g * q.s[i] : g;
    }
}

static constexpr int MIP_FLAGS = GSPL_MIP_RAW_SCALES | GSPL_MIP_RAW_OPACITIES | GSPL_MIP_COMPENSATE;
static constexpr int64_t MIP_MAX_N = 2147483647;

}  // namespace gspl

extern "C" int gspl_mip_filter3d(int64_t N, int C, const float* means, const float* cameras, float* filter_3d, float* distance,
                                 uint8_t* valid_any, void* workspace, void* stream) {
    using namespace gspl;
    if (N < 1 || N > MIP_MAX_N || C < 1) return fail_arg("mip_filter3d: N must be 1 .. 2^31 - 1 and C >= 1");
    if (!means || !cameras || !filter_3d || !workspace) return fail_arg("mip_filter3d: NULL required pointer");
    if ((reinterpret_cast<uintptr_t>(cameras) & 3u) || (reinterpret_cast<uintptr_t>(workspace) & 3u)) return fail_arg("mip_filter3d: misaligned pointer");
    int* stats = reinterpret_cast<int*>(workspace);
    if (const int e = check_hip(hipMemsetAsync(stats, 0, GSPL_MIP_WORKSPACE_BYTES, (hipStream_t)stream), "mip_filter3d: clearing the workspace")) return e;
    const int grid = (int)((N + MIP_BLOCK - 1) / MIP_BLOCK);
    hipLaunchKernelGGL(mip_filter3d_distance_kernel, dim3(grid), dim3(MIP_BLOCK), 0, (hipStream_t)stream, N, C, means, cameras, filter_3d,
                       distance, valid_any, stats);
    if (const int e = check_launch("mip_filter3d (distances)")) return e;
    hipLaunchKernelGGL(mip_filter3d_finish_kernel, dim3(grid), dim3(MIP_BLOCK), 0, (hipStream_t)stream, N, filter_3d, stats);
    return check_launch("mip_filter3d (filter)");
}

extern "C" int gspl_mip_apply_fwd(int64_t N, int flags, const float* scales, const float* opacities, const float* filter_3d,
                                  float* scales_out, float* opacities_out, void* stream) {
    using namespace gspl;
    if (N < 0 || N > MIP_MAX_N || (flags & ~MIP_FLAGS)) return fail_arg("mip_apply_fwd: bad N / flags");
    if ((flags & GSPL_MIP_RAW_OPACITIES) && !opacities) return fail_arg("mip_apply_fwd: RAW_OPACITIES without opacities");
    if (!opacities && !(flags & GSPL_MIP_COMPENSATE) && opacities_out) return fail_arg("mip_apply_fwd: no opacities and no COMPENSATE, but an opacities_out");
    if (N == 0) return GSPL_OK;
    if (!scales || !filter_3d || !scales_out || (opacities && !opacities_out)) return fail_arg("mip_apply_fwd: NULL required pointer");
    const int grid = (int)((N + MIP_BLOCK - 1) / MIP_BLOCK);
    dispatch_bools([&](auto rs, auto ro, auto comp) {
        hipLaunchKernelGGL((mip_apply_fwd_kernel<decltype(rs)::value, decltype(ro)::value, decltype(comp)::value>), dim3(grid), dim3(MIP_BLOCK), 0,
                           (hipStream_t)stream, N, scales, opacities, filter_3d, scales_out, opacities_out);
    }, (flags & GSPL_MIP_RAW_SCALES) != 0, (flags & GSPL_MIP_RAW_OPACITIES) != 0, (flags & GSPL_MIP_COMPENSATE) != 0);
    return check_launch("mip_apply_fwd");
}

extern "C" int gspl_mip_apply_bwd(int64_t N, int flags, const float* scales, const float* opacities, const float* filter_3d,
                                  const float* v_scales_out, const float* v_opacities_out, float* v_scales, float* v_opacities, void* stream) {
    using namespace gspl;
    if (N < 0 || N > MIP_MAX_N || (flags & ~MIP_FLAGS)) return fail_arg("mip_apply_bwd: bad N / flags");
    if ((flags & GSPL_MIP_RAW_OPACITIES) && !opacities) return fail_arg("mip_apply_bwd: RAW_OPACITIES without opacities");
    if (!opacities && v_opacities) return fail_arg("mip_apply_bwd: a v_opacities without opacities");
    if (!opacities && !(flags & GSPL_MIP_COMPENSATE) && v_opacities_out) return fail_arg("mip_apply_bwd: no opacities and no COMPENSATE, but a v_opacities_out");
    if (N == 0) return GSPL_OK;
    if (!scales || !filter_3d || !v_scales) return fail_arg("mip_apply_bwd: NULL required pointer");
    const int grid = (int)((N + MIP_BLOCK - 1) / MIP_BLOCK);
    dispatch_bools([&](auto rs, auto ro, auto comp) {
        hipLaunchKernelGGL((mip_apply_bwd_kernel<decltype(rs)::value, decltype(ro)::value, decltype(comp)::value>), dim3(grid), dim3(MIP_BLOCK), 0,
                           (hipStream_t)stream, N, scales, opacities, filter_3d, v_scales_out, v_opacities_out, v_scales, v_opacities);
    }, (flags & GSPL_MIP_RAW_SCALES) != 0, (flags & GSPL_MIP_RAW_OPACITIES) != 0, (flags & GSPL_MIP_COMPENSATE) != 0);
    return check_launch("mip_apply_bwd");
}

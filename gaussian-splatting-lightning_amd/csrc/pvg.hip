// pvg.hip — the vibration transform of Periodic Vibration Gaussians (gfx950, wave64); include/gspl_hip.h section 17.
//
// Chen et al., "Periodic Vibration Gaussian: Dynamic Urban Scene Reconstruction and Real-time Rendering": every Gaussian has a life
// peak t, a lifespan scale_t and a velocity; at the frame's time ts its mean swings around the stored one, its opacity is scaled by a
// Gaussian of (t - ts), and its average velocity over the lifespan is the velocity damped by the lifespan.  With a = 2 pi / cycle:
//     avg_velocity = velocity exp(-scale_t / cycle / 2 velocity_decay)
//     means_t      = means + velocity sin((ts - t) a) / a   (+ avg_velocity time_shift)
//     marginal     = exp(-0.5 (t - ts)^2 / scale_t^2),   opacity_t = opacities marginal
// One launch per direction, one lane per row: 36 B read and 28 B written forward, 64 B read and 36 B written backward (with all
// three upstream gradients).  The rows of the [N,3] arrays are read as three dwords per lane, so that the three load instructions of a
// wave cover the same 768 contiguous bytes; no LDS, no atomics.  sinf / cosf / expf are the accurate ones: the sine's argument
// reaches +-50 with the default cycle.  The per-call scalars come from a device table (ts is built from the camera's time tensor
// without a read-back): table[0] = ts, [1] = time_shift, [2] = 1 when shifted else 0, [3] = cycle, [4] = velocity_decay,
// [5] = a (2 pi / cycle evaluated in double by the caller: the kernel's own quotient of two rounded numbers would be an ulp worse).
#include "gspl_device.h"
#include "gspl_host.h"

namespace gspl {
namespace {

constexpr int kT = 256;

struct PvgScalars { float ts, shift, a, cycle, decay; bool shifted; };

__device__ inline PvgScalars load_scalars(const float* __restrict__ table) {
    PvgScalars s;
    s.ts = table[0];
    s.shift = table[1];
    s.shifted = table[2] != 0.f;
    s.cycle = table[3];
    s.decay = table[4];
    s.a = table[5];
    return s;
}

// marginal, and whether the row is alive: an underflowed (or undefined: scale_t^2 == 0 at t == ts) factor is exactly zero
__device__ inline float marginal_of(float t, float st, float ts, float* d_out) {
    const float d = t - ts;
    *d_out = d;
    const float m = expf(-0.5f * (d * d) / (st * st));
    return m > 0.f ? m : 0.f;      // NaN -> 0
}

// exp(-scale_t / cycle / 2 velocity_decay), in the order the model's getter evaluates it
__device__ inline float damping_of(float st, const PvgScalars& k) { return expf(-st / k.cycle * 0.5f * k.decay); }

__global__ __launch_bounds__(kT) void pvg_motion_fwd_kernel(int N, const float* __restrict__ means, const float* __restrict__ velocity,
                                                            const float* __restrict__ t, const float* __restrict__ scale_t,
                                                            const float* __restrict__ opacities, const float* __restrict__ table,
                                                            float* __restrict__ means_t, float* __restrict__ avg_velocity,
                                                            float* __restrict__ opacity_t) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= N) return;
    const PvgScalars k = load_scalars(table);
    const int64_t r = (int64_t)i * 3;
    const float ti = t[i], st = scale_t[i];
    const float e = damping_of(st, k);
    const float s = sinf((k.ts - ti) * k.a) / k.a;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = velocity[r + c], av = v * e;
        float m = means[r + c] + v * s;
        if (k.shifted) m += av * k.shift;
        avg_velocity[r + c] = av;
        means_t[r + c] = m;
    }
    float d;
    opacity_t[i] = opacities[i] * marginal_of(ti, st, k.ts, &d);
}

// All five gradients, every element written.  v_* nullable (= zero).  With M = marginal, G = v_avg_velocity + time_shift v_means_t:
//   g_means = v_means_t;   g_velocity = v_means_t sin(.) / a + G e;   g_opacities = v_opacity_t M
//   g_t       = -(v_means_t . velocity) cos((ts - t) a) - v_opacity_t opacities M (t - ts) / scale_t^2
//   g_scale_t = -(G . velocity) e velocity_decay / (2 cycle) + v_opacity_t opacities M (t - ts)^2 / scale_t^3
// Where M is zero its three terms are exactly zero (not 0 times an overflowed quotient).
__global__ __launch_bounds__(kT) void pvg_motion_bwd_kernel(int N, const float* __restrict__ velocity, const float* __restrict__ t,
                                                            const float* __restrict__ scale_t, const float* __restrict__ opacities,
                                                            const float* __restrict__ table, const float* __restrict__ v_means_t,
                                                            const float* __restrict__ v_avg_velocity, const float* __restrict__ v_opacity_t,
                                                            float* __restrict__ g_means, float* __restrict__ g_velocity, float* __restrict__ g_t,
                                                            float* __restrict__ g_scale_t, float* __restrict__ g_opacities) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= N) return;
    const PvgScalars k = load_scalars(table);
    const int64_t r = (int64_t)i * 3;
    const float ti = t[i], st = scale_t[i];
    const float e = damping_of(st, k);
    const float phase = (k.ts - ti) * k.a;
    const float s = sinf(phase) / k.a, co = cosf(phase);
    float gm_dot_v = 0.f, G_dot_v = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = velocity[r + c];
        const float gm = v_means_t ? v_means_t[r + c] : 0.f;
        float G = v_avg_velocity ? v_avg_velocity[r + c] : 0.f;
        if (k.shifted) G += gm * k.shift;
        g_means[r + c] = gm;
        g_velocity[r + c] = gm * s + G * e;
        gm_dot_v += gm * v;
        G_dot_v += G * v;
    }
    float d;
    const float M = marginal_of(ti, st, k.ts, &d);
    const float go = v_opacity_t ? v_opacity_t[i] : 0.f;
    float gt = -(gm_dot_v * co), gs = -(G_dot_v * e / k.cycle * 0.5f * k.decay), gop = 0.f;
    if (M > 0.f) {
        const float gM = go * opacities[i] * M;      // d L / d M times M
        const float q = gM * d / (st * st);      // (can overflow only where the fp32 torch formulation does)
        gt -= q;
        gs += q * d / st;
        gop = go * M;
    }
    g_t[i] = gt;
    g_scale_t[i] = gs;
    g_opacities[i] = gop;
}

}  // namespace
}  // namespace gspl

extern "C" int gspl_pvg_motion_fwd(int N, const float* means, const float* velocity, const float* t, const float* scale_t,
                                   const float* opacities, const float* table, float* means_t, float* avg_velocity, float* opacity_t,
                                   void* stream) {
    using namespace gspl;
    if (N < 0) return fail_arg("pvg_motion_fwd: N < 0");
    if (N == 0) return GSPL_OK;
    if (!means || !velocity || !t || !scale_t || !opacities || !table || !means_t || !avg_velocity || !opacity_t)
        return fail_arg("pvg_motion_fwd: NULL pointer");
    hipLaunchKernelGGL(pvg_motion_fwd_kernel, dim3((unsigned)(((int64_t)N + kT - 1) / kT)), dim3(kT), 0, (hipStream_t)stream, N, means, velocity, t,
                       scale_t, opacities, table, means_t, avg_velocity, opacity_t);
    return check_launch("pvg_motion_fwd");
}

extern "C" int gspl_pvg_motion_bwd(int N, const float* velocity, const float* t, const float* scale_t, const float* opacities,
                                   const float* table, const float* v_means_t, const float* v_avg_velocity, const float* v_opacity_t,
                                   float* g_means, float* g_velocity, float* g_t, float* g_scale_t, float* g_opacities, void* stream) {
    using namespace gspl;
    if (N < 0) return fail_arg("pvg_motion_bwd: N < 0");
    if (N == 0) return GSPL_OK;
    if (!velocity || !t || !scale_t || !opacities || !table || !g_means || !g_velocity || !g_t || !g_scale_t || !g_opacities)
        return fail_arg("pvg_motion_bwd: NULL pointer");
    hipLaunchKernelGGL(pvg_motion_bwd_kernel, dim3((unsigned)(((int64_t)N + kT - 1) / kT)), dim3(kT), 0, (hipStream_t)stream, N, velocity, t, scale_t,
                       opacities, table, v_means_t, v_avg_velocity, v_opacity_t, g_means, g_velocity, g_t, g_scale_t, g_opacities);
    return check_launch("pvg_motion_bwd");
}

// mcmc.hip — the per-step math of the 3DGS-MCMC density controller (gfx950, wave64); include/gspl_hip.h section 13.
//
// Kheradmand et al., "3D Gaussian Splatting as Markov Chain Monte Carlo".  The reference's controller
// (internal/density_controllers/mcmc_density_controller.py) calls three things per step or per event:
//   * relocation (Eq. 9): the opacity and scale a sampled Gaussian and its n - 1 copies get, `gsplat.relocation.compute_relocation`
//     in the reference (a CUDA kernel with no ROCm build) — relocation_kernel, one thread per row, binomials in LDS;
//   * the noise added to the means after every step (`_add_xyz_noise`, :93-119: compute_cov_3d, randn_like, a steep sigmoid, a
//     bmm — some thirty launches over 9-36 MB tensors) — perturb_kernel, ONE streaming launch with an in-register Philox4x32-10
//     generator, ~56 B of HBM traffic per Gaussian;
//   * the regulariser of internal/metrics/mcmc_metrics.py (`reg_loss`: two activated means) — reg_partials_kernel +
//     reg_final_kernel (deterministic two-level sum, no float atomics), reg_bwd_kernel (one elementwise launch).
#include "gspl_device.h"
#include "gspl_host.h"

namespace gspl {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxNMax = 64;           // binoms in LDS: 16 KB at most
constexpr int kRegMaxPartials = 1024;  // workgroups of the regulariser's first pass
constexpr int kRegRowsPerPartial = 4096;

// ---- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) ----------------------------------
struct U4 { uint32_t x, y, z, w; };

__device__ inline U4 philox_round(U4 c, uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    const uint32_t hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
    const uint32_t hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
    return U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
}

__device__ inline U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
    const uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        c = philox_round(c, k0, k1);
        k0 += W0;
        k1 += W1;
    }
    return philox_round(c, k0, k1);
}

// u32 -> (0, 1]: the top 24 bits plus one, times 2^-24 (exact in fp32; log never sees 0)
__device__ inline float u01(uint32_t b) { return (float)((b >> 8) + 1u) * 5.9604644775390625e-08f; }

// The counter layout of curand_init(seed, subsequence = i, offset) — what torch's own kernels use with the same generator: the block
// index offset / 4 in words 0-1, the subsequence (here the row) in words 2-3.  The caller has reserved offsets [offset, offset + 4)
// of the generator (offset a multiple of 4), so no torch kernel ever draws block offset / 4 of any subsequence.
__device__ inline U4 mcmc_bits(int64_t i, uint64_t seed, uint64_t offset) {
    const uint64_t blk = offset >> 2;
    const U4 ctr{(uint32_t)blk, (uint32_t)(blk >> 32), (uint32_t)(uint64_t)i, (uint32_t)((uint64_t)i >> 32)};
    return philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
}

__device__ inline void box_muller3(U4 b, float e[3]) {
    const float r01 = sqrtf(-2.f * logf(u01(b.x)));
    const float r23 = sqrtf(-2.f * logf(u01(b.z)));
    float s1, c1, s3, c3;
    sincospif(2.f * u01(b.y), &s1, &c1);      // 2u is exact: the angle carries no rounding of its own
    sincospif(2.f * u01(b.w), &s3, &c3);
    e[0] = r01 * c1;
    e[1] = r01 * s1;
    e[2] = r23 * c3;
}

// ---- relocation --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void relocation_kernel(int M, int n_max, const float* __restrict__ opacities, const float* __restrict__ scales,
                                                            const int32_t* __restrict__ ratios, const float* __restrict__ binoms,
                                                            float* __restrict__ new_opacities, float* __restrict__ new_scales) {
    __shared__ float sb[kMaxNMax * kMaxNMax];
    for (int j = threadIdx.x; j < n_max * n_max; j += kBlock) sb[j] = binoms[j];
    __syncthreads();
    const int m = blockIdx.x * kBlock + threadIdx.x;
    if (m >= M) return;
    const int n = min(max(ratios[m], 1), n_max);
    const float o = opacities[m];
    // 1 - (1 - o)^(1/n) without the cancellation of 1 - o for small o; n = 1 is the identity exactly
    const float x = n == 1 ? o : -expm1f(log1pf(-o) / (float)n);
    float denom = 0.f;
    for (int i = 1; i <= n; ++i) {
        float p = x;                                      // x^(k+1)
        for (int k = 0; k <= i - 1; ++k) {
            const float sgn_rsqrt = ((k & 1) ? -1.f : 1.f) / sqrtf((float)(k + 1));
            denom += sb[(i - 1) * n_max + k] * (sgn_rsqrt * p);
            p *= x;
        }
    }
    const float coeff = o / denom;
    new_opacities[m] = x;
#pragma unroll
    for (int c = 0; c < 3; ++c) new_scales[(size_t)m * 3 + c] = coeff * scales[(size_t)m * 3 + c];
}

// ---- noise on the means ----------------------------------------------------------------------------------------------------------
// One row: means += c(o) R diag(s^2) R^T eps, evaluated as R (s^2 * (R^T eps)).  R of internal/utils/gaussian_projection.py:211-232.
template <bool RAW>
__device__ inline void perturb_row(float m[3], const float s_in[3], const float q_in[4], float o_in, const float e[3], float coeff) {
    float s[3], q[4];
    float o = o_in;
    if (RAW) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = expf(s_in[c]);
        const float inv = 1.f / fmaxf(sqrtf(q_in[0] * q_in[0] + q_in[1] * q_in[1] + q_in[2] * q_in[2] + q_in[3] * q_in[3]), 1e-12f);
#pragma unroll
        for (int c = 0; c < 4; ++c) q[c] = q_in[c] * inv;
        o = 1.f / (1.f + expf(-o_in));
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = s_in[c];
#pragma unroll
        for (int c = 0; c < 4; ++c) q[c] = q_in[c];
    }
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    const float R[3][3] = {{1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y)},
                           {2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x)},
                           {2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)}};
    const float cs = coeff / (1.f + expf(-100.f * ((1.f - o) - 0.995f)));
    float v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = (R[0][k] * e[0] + R[1][k] * e[1] + R[2][k] * e[2]) * (s[k] * s[k]);
#pragma unroll
    for (int j = 0; j < 3; ++j) m[j] += cs * (R[j][0] * v[0] + R[j][1] * v[1] + R[j][2] * v[2]);
}

// Four rows per thread: with 16-byte aligned bases (VEC) every access is a 16-byte load / store — means, scales and noise are three
// float4 per four rows, rotations four, opacities one.  The last, incomplete group of rows (and unaligned bases) go row by row.
template <bool RAW>
__global__ __launch_bounds__(kBlock) void perturb_kernel(int N, float* __restrict__ means, const float* __restrict__ scales,
                                                         const float* __restrict__ rotations, const float* __restrict__ opacities,
                                                         const float* __restrict__ noise, float coeff, uint64_t seed, uint64_t offset, int vec) {
    const int64_t r0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 4;
    if (r0 >= N) return;
    const int cnt = (int)min((int64_t)4, (int64_t)N - r0);
    float m[12], s[12], q[16], o[4], e[12];
    if (vec && cnt == 4) {
        const float4* m4 = reinterpret_cast<const float4*>(means + r0 * 3);
        const float4* s4 = reinterpret_cast<const float4*>(scales + r0 * 3);
        const float4* q4 = reinterpret_cast<const float4*>(rotations + r0 * 4);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float4 a = m4[j], b = s4[j];
            m[4 * j] = a.x; m[4 * j + 1] = a.y; m[4 * j + 2] = a.z; m[4 * j + 3] = a.w;
            s[4 * j] = b.x; s[4 * j + 1] = b.y; s[4 * j + 2] = b.z; s[4 * j + 3] = b.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 a = q4[j];
            q[4 * j] = a.x; q[4 * j + 1] = a.y; q[4 * j + 2] = a.z; q[4 * j + 3] = a.w;
        }
        const float4 a = *reinterpret_cast<const float4*>(opacities + r0);
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
        if (noise) {
            const float4* e4 = reinterpret_cast<const float4*>(noise + r0 * 3);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float4 b = e4[j];
                e[4 * j] = b.x; e[4 * j + 1] = b.y; e[4 * j + 2] = b.z; e[4 * j + 3] = b.w;
            }
        }
    } else {
        for (int r = 0; r < cnt; ++r) {
            for (int c = 0; c < 3; ++c) {
                m[3 * r + c] = means[(r0 + r) * 3 + c];
                s[3 * r + c] = scales[(r0 + r) * 3 + c];
                if (noise) e[3 * r + c] = noise[(r0 + r) * 3 + c];
            }
            for (int c = 0; c < 4; ++c) q[4 * r + c] = rotations[(r0 + r) * 4 + c];
            o[r] = opacities[r0 + r];
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r < cnt) {
            if (!noise) box_muller3(mcmc_bits(r0 + r, seed, offset), e + 3 * r);
            perturb_row<RAW>(m + 3 * r, s + 3 * r, q + 4 * r, o[r], e + 3 * r, coeff);
        }
    }
    if (vec && cnt == 4) {
        float4* m4 = reinterpret_cast<float4*>(means + r0 * 3);
#pragma unroll
        for (int j = 0; j < 3; ++j) m4[j] = make_float4(m[4 * j], m[4 * j + 1], m[4 * j + 2], m[4 * j + 3]);
    } else {
        for (int r = 0; r < cnt; ++r)
            for (int c = 0; c < 3; ++c) means[(r0 + r) * 3 + c] = m[3 * r + c];
    }
}

__global__ __launch_bounds__(kBlock) void randn_kernel(int N, uint64_t seed, uint64_t offset, uint32_t* __restrict__ bits, float* __restrict__ normals) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const U4 b = mcmc_bits(i, seed, offset);
    if (bits) *reinterpret_cast<uint4*>(bits + i * 4) = make_uint4(b.x, b.y, b.z, b.w);
    float e[3];
    box_muller3(b, e);
    for (int c = 0; c < 3; ++c) normals[i * 3 + c] = e[c];
}

// ---- regulariser -----------------------------------------------------------------------------------------------------------------
__device__ inline float reg_o(float o, bool raw) { return raw ? 1.f / (1.f + expf(-o)) : fabsf(o); }
__device__ inline float reg_s(float s, bool raw) { return raw ? expf(s) : fabsf(s); }

// fixed-order tree sum of the workgroup's values a[0..kBlock).  The one workgroup sum that is not block_sum of gspl_reduce.h: an LDS tree
// associates differently from a butterfly and a chain over the waves, and the last bits of gspl_mcmc_reg_fwd's two scalars are its.
__device__ inline void block_sum2(float* a, float* b) {
#pragma unroll
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < w) {
            a[threadIdx.x] += a[threadIdx.x + w];
            b[threadIdx.x] += b[threadIdx.x + w];
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kBlock) void reg_partials_kernel(int N, int raw, const float* __restrict__ opacities, const float* __restrict__ scales,
                                                              float* __restrict__ partials) {
    __shared__ float so[kBlock], ss[kBlock];
    float ao = 0.f, as = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += (int64_t)gridDim.x * kBlock) {
        ao += reg_o(opacities[i], raw);
        as += reg_s(scales[i * 3], raw) + reg_s(scales[i * 3 + 1], raw) + reg_s(scales[i * 3 + 2], raw);
    }
    so[threadIdx.x] = ao;
    ss[threadIdx.x] = as;
    block_sum2(so, ss);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = so[0];
        partials[2 * blockIdx.x + 1] = ss[0];
    }
}

__global__ __launch_bounds__(kBlock) void reg_final_kernel(int N, int n_partials, const float* __restrict__ partials, float opacity_w, float scale_w,
                                                           float* __restrict__ out) {
    __shared__ float so[kBlock], ss[kBlock];
    float ao = 0.f, as = 0.f;
    for (int j = threadIdx.x; j < n_partials; j += kBlock) {
        ao += partials[2 * j];
        as += partials[2 * j + 1];
    }
    so[threadIdx.x] = ao;
    ss[threadIdx.x] = as;
    block_sum2(so, ss);
    if (threadIdx.x == 0) {
        out[0] = opacity_w * (so[0] / (float)N);
        out[1] = scale_w * (ss[0] / (3.f * (float)N));
    }
}

__global__ __launch_bounds__(kBlock) void reg_bwd_kernel(int N, int raw, const float* __restrict__ opacities, const float* __restrict__ scales,
                                                         float opacity_w, float scale_w, const float* __restrict__ grad_out,
                                                         float* __restrict__ v_opacities, float* __restrict__ v_scales) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const float go = grad_out[0] * opacity_w / (float)N, gs = grad_out[1] * scale_w / (3.f * (float)N);
    const float o = opacities[i];
    if (raw) {
        const float sg = 1.f / (1.f + expf(-o));
        v_opacities[i] = go * (sg * (1.f - sg));
    } else {
        v_opacities[i] = o > 0.f ? go : (o < 0.f ? -go : 0.f);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float s = scales[i * 3 + c];
        v_scales[i * 3 + c] = raw ? gs * expf(s) : (s > 0.f ? gs : (s < 0.f ? -gs : 0.f));
    }
}


}  // namespace
}  // namespace gspl

extern "C" int gspl_mcmc_relocation(int M, int n_max, const float* opacities, const float* scales, const int32_t* ratios, const float* binoms,
                                    float* new_opacities, float* new_scales, void* stream) {
    using namespace gspl;
    if (M < 0 || n_max < 1 || n_max > kMaxNMax) return fail_arg("mcmc_relocation: M >= 0 and 1 <= n_max <= 64");
    if (M == 0) return GSPL_OK;
    if (!opacities || !scales || !ratios || !binoms || !new_opacities || !new_scales) return fail_arg("mcmc_relocation: NULL pointer");
    hipLaunchKernelGGL(relocation_kernel, dim3((M + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, M, n_max, opacities, scales,
                       ratios, binoms, new_opacities, new_scales);
    return check_launch("mcmc_relocation");
}

extern "C" int gspl_mcmc_perturb_means(int N, int raw, float* means, const float* scales, const float* rotations, const float* opacities,
                                       const float* noise, float coeff, uint64_t seed, uint64_t offset, void* stream) {
    using namespace gspl;
    if (N < 0) return fail_arg("mcmc_perturb_means: N < 0");
    if (N == 0) return GSPL_OK;
    if (!means || !scales || !rotations || !opacities) return fail_arg("mcmc_perturb_means: NULL pointer");
    if (!noise && (offset & 3u)) return fail_arg("mcmc_perturb_means: the generator offset must be a multiple of 4");
    // (noise may be NULL: the kernel then draws its own, and NULL passes aligned16)
    const int vec = aligned16(means) && aligned16(scales) && aligned16(rotations) && aligned16(opacities) && aligned16(noise);
    const int64_t threads = ((int64_t)N + 3) / 4;
    const dim3 grid((unsigned)((threads + kBlock - 1) / kBlock));
    if (raw)
        hipLaunchKernelGGL(perturb_kernel<true>, grid, dim3(kBlock), 0, (hipStream_t)stream, N, means, scales, rotations, opacities, noise, coeff,
                           seed, offset, vec);
    else
        hipLaunchKernelGGL(perturb_kernel<false>, grid, dim3(kBlock), 0, (hipStream_t)stream, N, means, scales, rotations, opacities, noise, coeff,
                           seed, offset, vec);
    return check_launch("mcmc_perturb_means");
}

extern "C" int gspl_mcmc_randn(int N, uint64_t seed, uint64_t offset, uint32_t* bits, float* normals, void* stream) {
    using namespace gspl;
    if (N < 0) return fail_arg("mcmc_randn: N < 0");
    if (N == 0) return GSPL_OK;
    if (!normals || !aligned16(bits)) return fail_arg("mcmc_randn: NULL normals or bits not 16-byte aligned");
    if (offset & 3u) return fail_arg("mcmc_randn: the generator offset must be a multiple of 4");
    hipLaunchKernelGGL(randn_kernel, dim3((N + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, N, seed, offset, bits, normals);
    return check_launch("mcmc_randn");
}

extern "C" int gspl_mcmc_reg_partials(int N) {
    using namespace gspl;
    if (N <= 0) return 1;
    const int64_t g = ((int64_t)N + kRegRowsPerPartial - 1) / kRegRowsPerPartial;
    return (int)(g < kRegMaxPartials ? g : kRegMaxPartials);
}

extern "C" int gspl_mcmc_reg_fwd(int N, int raw, const float* opacities, const float* scales, float opacity_w, float scale_w,
                                 float* partials, float* out, void* stream) {
    using namespace gspl;
    if (N <= 0) return fail_arg("mcmc_reg_fwd: N must be positive (the mean of nothing is undefined)");
    if (!opacities || !scales || !partials || !out) return fail_arg("mcmc_reg_fwd: NULL pointer");
    const int G = gspl_mcmc_reg_partials(N);
    hipLaunchKernelGGL(reg_partials_kernel, dim3(G), dim3(kBlock), 0, (hipStream_t)stream, N, raw, opacities, scales, partials);
    int rc = check_launch("mcmc_reg_fwd");
    if (rc != GSPL_OK) return rc;
    hipLaunchKernelGGL(reg_final_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, N, G, partials, opacity_w, scale_w, out);
    return check_launch("mcmc_reg_fwd");
}

extern "C" int gspl_mcmc_reg_bwd(int N, int raw, const float* opacities, const float* scales, float opacity_w, float scale_w,
                                 const float* grad_out, float* v_opacities, float* v_scales, void* stream) {
    using namespace gspl;
    if (N < 0) return fail_arg("mcmc_reg_bwd: N < 0");
    if (N == 0) return GSPL_OK;
    if (!opacities || !scales || !grad_out || !v_opacities || !v_scales) return fail_arg("mcmc_reg_bwd: NULL pointer");
    hipLaunchKernelGGL(reg_bwd_kernel, dim3((N + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, N, raw, opacities, scales,
                       opacity_w, scale_w, grad_out, v_opacities, v_scales);
    return check_launch("mcmc_reg_bwd");
}

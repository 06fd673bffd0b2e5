// glossy.hip — the view-dependent opacity of the Glossy-Gaussian route, forward and backward (gfx950; include/gspl_hip.h section 25).
//
// Restates internal/renderers/glossy_renderer.py `GlossyRendererModule.get_opacities` and internal/models/glossy_gaussian.py
// `get_view_dep_opacities`: F.normalize(means - camera) -> eval_sh_decomposed(degree, opacities, opacity_rest, d) + 0.5 -> clamp(0, 1),
// one channel.  The basis is sh_basis of gspl_device.h (internal/utils/sh_utils.py:133-170; the same polynomial forms, so they agree
// with the reference for the non-unit argument d = 0 too).
//
// Roofline: HBM-bound, 12 + 4 + 4 n_rest bytes read and 4 written per row forward; the backward reads 4 more and writes 4 + 4 n_rest.
// A `rest` row is 4 n_rest bytes (60 for degree 3): a lane-per-row read would touch 30 cache lines per wave instruction.  As in sh.hip
// a workgroup streams its 256 rows as one flat coalesced copy into LDS rows of ODD stride (lane r then reads row r without a bank
// conflict), and the backward stores its gradient rows the same way in reverse.  No atomics, no scratch, nothing saved by the forward.
// (tile_load / tile_store of gspl_rowtile.h, shared with sh.hip; tile_load's PART form leaves out the columns above the active degree
// and the rows without an incoming gradient.)
//
// Contraction as the language defines it: both kernels evaluate `raw` through the one function below and must agree on its bits (the
// backward decides the clamp on the value it recomputes).
#pragma clang fp contract(on)
#include "gspl_device.h"
#include "gspl_host.h"
#include "gspl_rowtile.h"

namespace gspl {

static constexpr int GLOSSY_BLOCK = 256;          // rows (= threads) per workgroup
static constexpr int GLOSSY_MAX_REST = 61;        // the backward's flags + 256 rows x 61 floats + the block vote's 256 bytes fit 64 KiB
                                                  // of LDS (the reference's widest row is 24)

// d = v / max(|v|, 1e-12) (F.normalize: the zero vector stays zero), then the basis values b[0 .. K)
template <int DEG>
__device__ __forceinline__ void glossy_basis(const float* __restrict__ means, const float* __restrict__ origin, int64_t n, float* b) {
    const float vx = means[n * 3 + 0] - origin[0], vy = means[n * 3 + 1] - origin[1], vz = means[n * 3 + 2] - origin[2];
    const float inv = 1.f / fmaxf(sqrtf(vx * vx + vy * vy + vz * vz), 1e-12f);
    sh_basis(DEG, vx * inv, vy * inv, vz * inv, b);
}

// C0 dc + sum_k b[k] rest[k - 1] + 0.5: ONE fmaf chain in k order
template <int DEG>
__device__ __forceinline__ float glossy_raw(const float* b, float dc, const float* row) {
    constexpr int K = (DEG + 1) * (DEG + 1);
    float acc = b[0] * dc;
#pragma unroll
    for (int k = 1; k < K; ++k) acc = fmaf(b[k], row[k - 1], acc);
    return acc + 0.5f;
}

template <int DEG>
__global__ __launch_bounds__(GLOSSY_BLOCK) void sh_opacity_fwd_kernel(
    int N, int n_rest, const float* __restrict__ means, const float* __restrict__ origin, const float* __restrict__ dc,
    const float* __restrict__ rest, int vec_ok, float* __restrict__ opacities) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int K = (DEG + 1) * (DEG + 1);
    constexpr int ls = (K - 1) | 1;
    const int64_t n0 = (int64_t)blockIdx.x * GLOSSY_BLOCK;
    const int rows = (int)min((int64_t)GLOSSY_BLOCK, (int64_t)N - n0);
    if (DEG > 0) {
        tile_load<GLOSSY_BLOCK, 1, true>(rest + n0 * n_rest, rows, n_rest, ls, 1.f / (float)(K - 1), lds, vec_ok != 0, K - 1);
        __syncthreads();
    }
    const int r = threadIdx.x;
    if (r >= rows) return;
    const int64_t n = n0 + r;
    float b[K];
    glossy_basis<DEG>(means, origin, n, b);
    const float raw = glossy_raw<DEG>(b, dc[n], lds + r * ls);
    opacities[n] = raw < 0.f ? 0.f : (raw > 1.f ? 1.f : raw);      // (a NaN stays one, as under torch.clamp)
}

// LDS: [0, 256) the rows' flags (incoming gradient non-zero), then 256 rows of stride ls = n_rest | 1: the staged coefficients first,
// the gradient rows afterwards (lane r reads and then overwrites row r only).
template <int DEG>
__global__ __launch_bounds__(GLOSSY_BLOCK) void sh_opacity_bwd_kernel(
    int N, int n_rest, const float* __restrict__ means, const float* __restrict__ origin, const float* __restrict__ dc,
    const float* __restrict__ rest, const float* __restrict__ v_opacities, int vec_in, int vec_out,
    float* __restrict__ v_dc, float* __restrict__ v_rest) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int K = (DEG + 1) * (DEG + 1);
    int* live = reinterpret_cast<int*>(lds);
    float* tile = lds + GLOSSY_BLOCK;
    const int ls = n_rest | 1;
    const int64_t n0 = (int64_t)blockIdx.x * GLOSSY_BLOCK;
    const int rows = (int)min((int64_t)GLOSSY_BLOCK, (int64_t)N - n0);
    const int r = threadIdx.x;
    const int64_t n = n0 + r;
    const float v = r < rows ? v_opacities[n] : 0.f;
    const int mine = v != 0.f;                                      // (a NaN gradient is one)
    live[r] = mine;
    const int any = __syncthreads_or(mine);
    if (DEG > 0 && any) {
        tile_load<GLOSSY_BLOCK, 1, true>(rest + n0 * n_rest, rows, n_rest, ls, 1.f / (float)(K - 1), tile, vec_in != 0, K - 1, live);
        __syncthreads();
    }
    if (r < rows) {
        float b[K];
#pragma unroll
        for (int k = 0; k < K; ++k) b[k] = 0.f;
        float g = 0.f;
        if (mine) {
            glossy_basis<DEG>(means, origin, n, b);
            const float raw = glossy_raw<DEG>(b, dc[n], tile + r * ls);
            g = (raw >= 0.f && raw <= 1.f) ? v : 0.f;               // torch.clamp's rule: both ends pass
        }
        const bool pass = g != 0.f;
        v_dc[n] = pass ? b[0] * g : 0.f;
        float* row = tile + r * ls;
#pragma unroll
        for (int k = 1; k < K; ++k) row[k - 1] = pass ? b[k] * g : 0.f;
        for (int j = K - 1; j < n_rest; ++j) row[j] = 0.f;          // above the active degree
    }
    if (n_rest > 0) {
        __syncthreads();
        tile_store<GLOSSY_BLOCK>(v_rest + n0 * n_rest, rows, n_rest, ls, 1.f / (float)n_rest, tile, vec_out != 0);
    }
}

static int glossy_check(const char* who, int N, int degree, int n_rest) {
    if (N < 0 || degree < 0 || degree > 4) return fail_arg(who);
    if (n_rest < (degree + 1) * (degree + 1) - 1 || n_rest > GLOSSY_MAX_REST) return fail_arg(who);
    return GSPL_OK;
}

}  // namespace gspl

extern "C" int gspl_sh_opacity_fwd(int N, int degree, int n_rest, const float* means, const float* origin, const float* dc,
                                   const float* rest, float* opacities, void* stream) {
    using namespace gspl;
    if (const int e = glossy_check("sh_opacity_fwd: bad N / degree / n_rest", N, degree, n_rest)) return e;
    if (N == 0) return GSPL_OK;
    if (!means || !origin || !dc || !opacities || ((n_rest > 0) != (rest != nullptr))) return fail_arg("sh_opacity_fwd: NULL required pointer (rest is NULL iff n_rest == 0)");
    const int K = (degree + 1) * (degree + 1);
    // every block starts 256 n_rest floats further on, a multiple of 16 bytes: only the base matters
    const int vec_ok = (degree > 0 && aligned16(rest)) ? 1 : 0;
    const size_t lds_bytes = degree > 0 ? (size_t)GLOSSY_BLOCK * ((K - 1) | 1) * sizeof(float) : 0;
    const int grid = (int)(((int64_t)N + GLOSSY_BLOCK - 1) / GLOSSY_BLOCK);
    dispatch_int<0, 1, 2, 3, 4>(degree, [&](auto deg) {
        hipLaunchKernelGGL(sh_opacity_fwd_kernel<decltype(deg)::value>, dim3(grid), dim3(GLOSSY_BLOCK), lds_bytes, (hipStream_t)stream, N, n_rest,
                           means, origin, dc, rest, vec_ok, opacities);
    });
    return check_launch("sh_opacity_fwd");
}

extern "C" int gspl_sh_opacity_bwd(int N, int degree, int n_rest, const float* means, const float* origin, const float* dc,
                                   const float* rest, const float* v_opacities, float* v_dc, float* v_rest, void* stream) {
    using namespace gspl;
    if (const int e = glossy_check("sh_opacity_bwd: bad N / degree / n_rest", N, degree, n_rest)) return e;
    if (N == 0) return GSPL_OK;
    if (!means || !origin || !dc || !v_opacities || !v_dc || ((n_rest > 0) != (rest != nullptr)) || ((n_rest > 0) != (v_rest != nullptr)))
        return fail_arg("sh_opacity_bwd: NULL required pointer (rest and v_rest are NULL iff n_rest == 0)");
    const int vec_in = (degree > 0 && aligned16(rest)) ? 1 : 0;
    const int vec_out = (n_rest > 0 && aligned16(v_rest)) ? 1 : 0;
    const size_t lds_bytes = (size_t)GLOSSY_BLOCK * (1 + (n_rest | 1)) * sizeof(float);      // 62 KiB at n_rest = 61
    const int grid = (int)(((int64_t)N + GLOSSY_BLOCK - 1) / GLOSSY_BLOCK);
    dispatch_int<0, 1, 2, 3, 4>(degree, [&](auto deg) {
        hipLaunchKernelGGL(sh_opacity_bwd_kernel<decltype(deg)::value>, dim3(grid), dim3(GLOSSY_BLOCK), lds_bytes, (hipStream_t)stream, N, n_rest,
                           means, origin, dc, rest, v_opacities, vec_in, vec_out, v_dc, v_rest);
    });
    return check_launch("sh_opacity_bwd");
}

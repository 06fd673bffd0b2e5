// adam.hip — visibility-masked fused Adam over all per-Gaussian parameter tensors in one launch (gfx950).
//
// "Next" row of SURVEY.md §8f (rank 3).  Replaces gsplat's `SelectiveAdam` (un-vendored; reference wrapper
// internal/optimizers.py:26-58, enabled by configs/gsplat_v1-accel_more.yaml) and, with the mask absent and bias
// correction on, the per-tensor `torch.optim.Adam` steps of the default configuration
// (internal/models/vanilla_gaussian.py:266-300: one parameter group per property, eps 1e-15).
// Update restated (the published selective_adam kernel): for every element of every row n with visible[n]
//     m = b1 m + (1 - b1) g;   v = b2 v + (1 - b2) g^2;   p -= step * m / (sqrt(v) * inv_bc2 + eps)
// with step = lr, inv_bc2 = 1 (gsplat: no bias correction) or step = lr / (1 - b1^t), inv_bc2 = 1 / sqrt(1 - b2^t)
// (torch.optim.Adam).  Rows with visible[n] == 0 keep parameter AND moments untouched.
//
// HBM-bound: 28 B per updated element (p, g, m, v read; p, m, v written).  All tensors of the model go through one
// launch (blockIdx.y = tensor); lanes handle 16-byte chunks of the flat [N * row] arrays, the row's visibility is looked
// up per element (byte loads, cache resident).
//
// grad_rows (gspl_selective_adam_rows): one byte per row, 0 = every gradient of the row is zero (the sparse tail of the fused Inria
// backward leaves it).  Every row is still updated — moments decay and parameters move with g = 0, as torch.optim.Adam has it — but a
// 16-byte chunk whose rows all carry 0 does not LOAD its gradient: adam_elem runs on a zero that arrives as a kernel argument, the same
// instructions on the same values.  Applied to tensors of at least GSPL_ADAM_ROWS_MIN floats per row, where whole cache lines of the
// gradient go unread; the 1-4 float tensors touch most of their lines at any density and are read as always.
//
// Rows that never had a gradient (zero moments, zero gradient) are passed over, chunk by chunk in the wide tensors and 128-byte line by
// line in the narrow ones: see selective_adam_kernel.
#include <cmath>
#include <cstdlib>

#include "gspl_device.h"
#include "gspl_host.h"
#include "gspl_rowtile.h"

namespace gspl {

struct AdamTensorDev {
    float* p;
    const float* g;
    float* m;
    float* v;
    float lr;
    int row;          // elements per Gaussian
};
struct AdamBatchDev { AdamTensorDev t[GSPL_ADAM_MAX_TENSORS]; };

// (adam_elem: gspl_device.h — shared with the backward kernels that apply the update themselves)

#ifndef GSPL_ADAM_ROWS_MIN
#define GSPL_ADAM_ROWS_MIN 32      // floats per row: one 128-byte line
#endif
// No-op chunks (SKIP): a row no view has ever blended has m = v = +0 (as the optimizers create them) and g = +-0, and adam_elem then
// gives m' = fma(b1, +0, (1 - b1) g) = +0, v' = +0, p' = p - (step * +0) / fma(0, inv_bc2, eps) = p - (+0) = p: the bits of all three stay
// as they are for EVERY p (-0, denormals, inf, quiet NaN), provided eps > 0, b1 and b2 in [0, 1], step finite and >= +0 (a step of -0
// would turn p = -0 into +0) and inv_bc2 finite — the host decides that once per launch (gspl_selective_adam_rows).  Such a chunk
// loads neither p nor stores anything: m, v (and g, where it is read at all) arrive first, p follows for the chunks that are live.
// m and v are compared as BITS: a moment of -0 is no no-op, the update turns it into +0.  Everything else runs the code it always ran.
template <bool ROWS, bool SKIP>
__global__ __launch_bounds__(256) void selective_adam_kernel(AdamBatchDev batch, int N, const uint8_t* __restrict__ visible,
                                                             float b1, float b2, float eps, float inv_bc1, float inv_bc2,
                                                             const uint8_t* __restrict__ grad_rows, float zero) {
    const AdamTensorDev T = batch.t[blockIdx.y];
    const int64_t total = (int64_t)N * T.row;
    const float step = T.lr * inv_bc1;
    const int64_t nvec = total >> 2;
    // the dense form: two 16-byte chunks per thread and iteration (8 loads in flight) and streaming (nontemporal) accesses of everything
    // that is not read again before the next step: 302 -> 257 us at 1 M Gaussians (1.65 GB: 6.4 TB/s).  The skipping form takes ONE
    // chunk: a live chunk makes two dependent round trips, and what hides the second is other waves — 44 registers and 8 waves per SIMD
    // against 79 and 6 with two chunks (three: 108 and 4, four: 134 and 3).  Measured at S-1080p-1M on one lease, the dense form at
    // 239 us: 194 / 207 / 249 us with one / two / three chunks, 311 with four on another lease (profiles/adam_noop_rows.txt).  The
    // loads keep the dense form's order (row flags, then g, m and v together): asking for m and v ahead of the flags was 5 - 8 us slower
    constexpr int U = SKIP ? 1 : 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // the rows of a chunk with ONE division per chunk, a 32-bit one wherever the tensor has fewer than 2^31 elements (a chunk of 4
    // floats of a row of >= 32 lies in one row or two)
    // Tensors of fewer than GSPL_ADAM_ROWS_MIN floats per row decide per GROUP OF 8 LANES, the 8 chunks of 128 bytes: a line of theirs holds
    // 8 - 32 rows, and passing over single chunks left p loads and stores that touched a part of nearly every line.  If one chunk of the group
    // is live, all 8 take the update (a no-op chunk gets the bits it had: the proof above) and the stores are whole lines; a group without a
    // live chunk is passed over as before.  The five narrow tensors of the model at 1 M rows, launch alone: 87.5 -> 63.6 us at 23 % live rows,
    // 55.8 -> 48.7 us at 5 %, 67.6 -> 66.0 us with every row live (profiles/adam_live_tiles.txt).
    const bool wide = T.row >= GSPL_ADAM_ROWS_MIN;
    const bool use_rows = ROWS && wide;
    const bool narrow = total < ((int64_t)1 << 31);
    auto has_grad = [&](int64_t e) {
        int64_t r0;
        int rem;
        if (narrow) { const uint32_t q = (uint32_t)e / (uint32_t)T.row; r0 = q; rem = (int)((uint32_t)e - q * (uint32_t)T.row); }
        else { r0 = e / T.row; rem = (int)(e - r0 * T.row); }
        return grad_rows[r0] != 0 || (rem + 3 >= T.row && grad_rows[r0 + 1] != 0);
    };
    auto still = [](bool vis, float g, float m, float v) { return !vis || (((__float_as_uint(m) | __float_as_uint(v)) == 0u) && g == 0.f); };
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < nvec; i0 += U * stride) {
        float4 p[U], g[U], m[U], v[U];
        bool vis[U][4], any[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            any[u] = false;
            if (i < nvec) {
                const int64_t e = i << 2;
#pragma unroll
                for (int k = 0; k < 4; ++k) { vis[u][k] = visible ? visible[(e + k) / T.row] != 0 : true; any[u] = any[u] || vis[u][k]; }
            }
            if (any[u]) {
                if (!SKIP) p[u] = load16_nt(T.p, i);
                if (!use_rows || has_grad(i << 2)) g[u] = load16_nt(T.g, i);
                else g[u] = make_float4(zero, zero, zero, zero);
                m[u] = load16_nt(T.m, i);
                v[u] = load16_nt(T.v, i);
            }
        }
        if (SKIP) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool quiet = !any[u] || (still(vis[u][0], g[u].x, m[u].x, v[u].x) && still(vis[u][1], g[u].y, m[u].y, v[u].y) &&
                                               still(vis[u][2], g[u].z, m[u].z, v[u].z) && still(vis[u][3], g[u].w, m[u].w, v[u].w));
                bool pass = quiet;
                if (!wide) {       // (uniform in the workgroup: every lane still in the loop takes part in the ballot)
                    const unsigned long long live = __ballot(!quiet);
                    pass = ((live >> (threadIdx.x & 56)) & 0xffull) == 0ull;
                }
                if (!any[u]) continue;
                if (pass) any[u] = false;
                else p[u] = load16_nt(T.p, i0 + u * stride);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!any[u]) continue;
            const int64_t i = i0 + u * stride;
            if (vis[u][0]) adam_elem(p[u].x, g[u].x, m[u].x, v[u].x, step, b1, b2, inv_bc2, eps);
            if (vis[u][1]) adam_elem(p[u].y, g[u].y, m[u].y, v[u].y, step, b1, b2, inv_bc2, eps);
            if (vis[u][2]) adam_elem(p[u].z, g[u].z, m[u].z, v[u].z, step, b1, b2, inv_bc2, eps);
            if (vis[u][3]) adam_elem(p[u].w, g[u].w, m[u].w, v[u].w, step, b1, b2, inv_bc2, eps);
            reinterpret_cast<float4*>(T.p)[i] = p[u];
            store16_nt(T.m, i, m[u]);
            store16_nt(T.v, i, v[u]);
        }
    }
    // tail (total not a multiple of 4)
    if (blockIdx.x == 0) {
        for (int64_t e = (nvec << 2) + threadIdx.x; e < total; e += blockDim.x) {
            if (visible && visible[e / T.row] == 0) continue;
            float p = T.p[e], m = T.m[e], v = T.v[e];
            adam_elem(p, T.g[e], m, v, step, b1, b2, inv_bc2, eps);
            T.p[e] = p; T.m[e] = m; T.v[e] = v;
        }
    }
}

}  // namespace gspl

extern "C" int gspl_selective_adam(int n_tensors, const gspl_adam_tensor* tensors, int N, const uint8_t* visible,
                                   float beta1, float beta2, float eps, float bias_correction1, float bias_correction2_sqrt,
                                   void* stream) {
    return gspl_selective_adam_limited(n_tensors, tensors, N, visible, beta1, beta2, eps, bias_correction1, bias_correction2_sqrt, 0, stream);
}

extern "C" int gspl_selective_adam_limited(int n_tensors, const gspl_adam_tensor* tensors, int N, const uint8_t* visible,
                                           float beta1, float beta2, float eps, float bias_correction1, float bias_correction2_sqrt,
                                           int max_blocks, void* stream) {
    return gspl_selective_adam_rows(n_tensors, tensors, N, visible, nullptr, beta1, beta2, eps, bias_correction1, bias_correction2_sqrt, max_blocks, stream);
}

extern "C" int gspl_selective_adam_rows(int n_tensors, const gspl_adam_tensor* tensors, int N, const uint8_t* visible, const uint8_t* grad_rows,
                                        float beta1, float beta2, float eps, float bias_correction1, float bias_correction2_sqrt,
                                        int max_blocks, void* stream) {
    using namespace gspl;
    if (max_blocks < 0) return fail_arg("selective_adam: bad sizes");
    if (n_tensors < 0 || n_tensors > GSPL_ADAM_MAX_TENSORS || N < 0) return fail_arg("selective_adam: bad sizes");
    if (n_tensors == 0 || N == 0) return GSPL_OK;
    if (!tensors) return fail_arg("selective_adam: NULL tensor table");
    if (!(bias_correction1 > 0.f) || !(bias_correction2_sqrt > 0.f)) return fail_arg("selective_adam: bias corrections must be positive (1 = none)");
    AdamBatchDev b;
    int64_t longest = 0;
    for (int k = 0; k < n_tensors; ++k) {
        const gspl_adam_tensor& t = tensors[k];
        if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq || t.row_elems <= 0) return fail_arg("selective_adam: bad tensor entry");
        if ((((uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq) & 15u) != 0)
            return fail_arg("selective_adam: tensors must be 16-byte aligned");
        b.t[k] = AdamTensorDev{t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.lr, t.row_elems};
        longest = std::max<int64_t>(longest, (int64_t)N * t.row_elems);
    }
    for (int k = n_tensors; k < GSPL_ADAM_MAX_TENSORS; ++k) b.t[k] = b.t[0];
    const int64_t want = ((longest >> 2) + 255) / 256;
    // max_blocks > 0: a launch that runs NEXT TO other work (the deferred update on the colour stream) keeps to that many workgroups
    // per tensor, so that it leaves wave slots on every CU to the kernels of the other stream; the loop is grid-strided either way
    const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(want, max_blocks > 0 ? max_blocks : 16384));
    // the range in which a chunk of zero moments and zero gradients is a no-op (the kernel's header); the products as the kernel forms them.
    // GSPL_ADAM_SKIP_NOOP=0 (read once): every chunk takes the dense path — the same values, what the tests compare against
    static const bool skip_enabled = [] { const char* e = getenv("GSPL_ADAM_SKIP_NOOP"); return !(e && e[0] == '0' && e[1] == 0); }();
    const float inv_bc1 = 1.f / bias_correction1, inv_bc2 = 1.f / bias_correction2_sqrt;
    bool skip = skip_enabled && eps > 0.f && beta1 >= 0.f && beta1 <= 1.f && beta2 >= 0.f && beta2 <= 1.f && std::isfinite(inv_bc2);
    for (int k = 0; k < n_tensors && skip; ++k) {
        const float step = tensors[k].lr * inv_bc1;
        skip = std::isfinite(step) && step >= 0.f && !std::signbit(step);
    }
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(gx, n_tensors), dim3(256), 0, (hipStream_t)stream, b, N, visible,
                           beta1, beta2, eps, inv_bc1, inv_bc2, grad_rows, 0.f);
    };
    if (grad_rows) { if (skip) launch(selective_adam_kernel<true, true>); else launch(selective_adam_kernel<true, false>); }
    else { if (skip) launch(selective_adam_kernel<false, true>); else launch(selective_adam_kernel<false, false>); }
    return check_launch("selective_adam");
}

// depthloss.hip — the depth-regularisation loss (gfx950, wave64); include/gspl_hip.h section 29.
//
// What `HasInverseDepthMetricsModule.get_inverse_depth_metric` (internal/metrics/inverse_depth_metrics.py:70-104) and
// `DepthMetricsModule.get_inverse_depth_metric` (internal/metrics/depth_metrics.py:52-61) compute from a predicted [H, W] map and the
// data set's: an optional normalisation, up to two masks multiplied into both sides, and mean |gt - pred| or mean (gt - pred)^2 over all
// H W elements.  In torch that is six to ten launches over the map in each direction; here
//   forward   depth_stats_kernel (only for the normalisations that need a number first: min / max of pred, or mean of gt), then
//             depth_loss_fwd_kernel: the elementwise pass with one partial sum per workgroup;
//   backward  depth_loss_bwd_kernel, elementwise.
// Both forward kernels finish INSIDE their launch: the workgroup that arrives last at a counter adds (or min / maxes) all partials in
// index order, whichever workgroup that is, so two runs give the same bits and no float atomic is used.  Each partial is stored and
// read with agent-scope atomics, the counter is an acquire-release add: the last arriver's reads happen after every other
// workgroup's store on any XCD.  The host clears the two counters with a 16-byte memset node before the launches and reads nothing.
#include "gspl_device.h"
#include "gspl_host.h"
#include "gspl_reduce.h"

namespace gspl {
namespace {

constexpr int DL_BLOCK = 256;
constexpr int DL_CHAIN = 8;                          // elements per thread of a partial
constexpr int DL_PER_PARTIAL = DL_BLOCK * DL_CHAIN;
constexpr int64_t DL_MAX = (int64_t)1 << 31;         // elements; 2^31 / 2048 partials at the most

struct DlMasks { const void* gt_mask; const void* pixel_mask; int gt_mask_u8, pixel_mask_u8; };
__device__ __forceinline__ float mask_at(const void* m, int u8, int64_t q) {
    return u8 ? (float)((const uint8_t*)m)[q] : ((const float*)m)[q];
}

// stats[0], stats[1]: MINMAX -> min and max of pred; MEAN -> mean of gt (one true division of the sum by H W), 0.
struct DlNorm { int kind; const float* stats; const float* median; float median_value; };

// gt' and pred' as the reference forms them, every operation rounded on its own: the normalisation, then gt_mask, then pixel_mask on
// both sides.  `scale` = d pred' / d pred.
__device__ __forceinline__ void normalised_pair(const DlNorm& nm, const DlMasks& mk, int64_t q, float p, float g, float& gn, float& pn, float& scale) {
#pragma clang fp contract(off)
    gn = g; pn = p; scale = 1.f;
    if (nm.kind == GSPL_DEPTH_NORM_MINMAX) {
        const float mn = nm.stats[0], den = (nm.stats[1] - mn) + 1e-8f;
        pn = (p - mn) / den; scale = 1.f / den;
    } else if (nm.kind == GSPL_DEPTH_NORM_MEDIAN) {
        const float med = nm.median ? nm.median[0] : nm.median_value;
        pn = p / med; scale = 1.f / med;
    } else if (nm.kind == GSPL_DEPTH_NORM_MEAN) {
        const float mean = nm.stats[0];
        gn = g / mean; pn = p / mean; scale = 1.f / mean;
    }
    if (mk.gt_mask) { const float m = mask_at(mk.gt_mask, mk.gt_mask_u8, q); gn *= m; pn *= m; scale *= m; }
    if (mk.pixel_mask) { const float m = mask_at(mk.pixel_mask, mk.pixel_mask_u8, q); gn *= m; pn *= m; scale *= m; }
}

// The last workgroup to arrive (true for all of its threads): every workgroup's partial stores, made by its thread 0 before this call,
// are visible to it.  `counter` is zero before the launch.
__device__ __forceinline__ bool arrives_last(uint32_t* counter) {
    __shared__ bool last;
    if (threadIdx.x == 0)
        last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    __syncthreads();
    if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return last;
}
__device__ __forceinline__ void put(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float get(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}

// MINMAX: partials[2 b], [2 b + 1] = min, max of pred over the workgroup's elements (min / max are exact: any order gives the same
// bits; NaN elements are passed over, as fminf does).  MEAN: partials[b] = the sum of gt, block_sum's order.
template <bool MINMAX>
__global__ __launch_bounds__(DL_BLOCK) void depth_stats_kernel(int64_t P, const float* __restrict__ x, float* partials, uint32_t* counter,
                                                               float* __restrict__ stats) {
    __shared__ float sh[DL_BLOCK / 64], sh2[DL_BLOCK / 64];
    const int64_t base = (int64_t)blockIdx.x * DL_PER_PARTIAL + threadIdx.x;
    float a = MINMAX ? INFINITY : 0.f, b = -INFINITY;
    for (int k = 0; k < DL_CHAIN; ++k) {
        const int64_t q = base + (int64_t)k * DL_BLOCK;
        if (q >= P) break;
        const float v = x[q];
        if (MINMAX) { a = fminf(a, v); b = fmaxf(b, v); }
        else a += v;
    }
    const int n = gridDim.x;
    if (MINMAX) {
        a = wave_min(a); b = -wave_min(-b);
        if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = a; sh2[threadIdx.x >> 6] = b; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < DL_BLOCK / 64; ++w) { a = fminf(a, sh[w]); b = fmaxf(b, sh2[w]); }
            put(partials + 2 * blockIdx.x, a); put(partials + 2 * blockIdx.x + 1, b);
        }
        if (!arrives_last(counter)) return;
        a = INFINITY; b = -INFINITY;
        for (int k = threadIdx.x; k < n; k += DL_BLOCK) { a = fminf(a, get(partials + 2 * k)); b = fmaxf(b, get(partials + 2 * k + 1)); }
        a = wave_min(a); b = -wave_min(-b);
        if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = a; sh2[threadIdx.x >> 6] = b; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < DL_BLOCK / 64; ++w) { a = fminf(a, sh[w]); b = fmaxf(b, sh2[w]); }
            stats[0] = a; stats[1] = b;
        }
    } else {
        const float total = block_sum<DL_BLOCK>(a, sh);
        if (threadIdx.x == 0) put(partials + blockIdx.x, total);
        if (!arrives_last(counter)) return;
        float acc = 0.f;
        for (int k = threadIdx.x; k < n; k += DL_BLOCK) acc += get(partials + k);
        const float sum = block_sum<DL_BLOCK>(acc, sh);
        if (threadIdx.x == 0) { stats[0] = sum / (float)P; stats[1] = 0.f; }
    }
}

template <bool L2>
__global__ __launch_bounds__(DL_BLOCK) void depth_loss_fwd_kernel(int64_t P, const float* __restrict__ pred, const float* __restrict__ gt,
                                                                  DlNorm nm, DlMasks mk, float* partials, uint32_t* counter, float* __restrict__ out) {
    __shared__ float sh[DL_BLOCK / 64];
    const int64_t base = (int64_t)blockIdx.x * DL_PER_PARTIAL + threadIdx.x;
    float acc = 0.f;
    for (int k = 0; k < DL_CHAIN; ++k) {
        const int64_t q = base + (int64_t)k * DL_BLOCK;
        if (q >= P) break;
        float gn, pn, scale;
        normalised_pair(nm, mk, q, pred[q], gt[q], gn, pn, scale);
        const float d = gn - pn;
        acc = L2 ? fmaf(d, d, acc) : acc + fabsf(d);
    }
    const float total = block_sum<DL_BLOCK>(acc, sh);
    if (threadIdx.x == 0) put(partials + blockIdx.x, total);
    if (!arrives_last(counter)) return;
    const int n = gridDim.x;
    acc = 0.f;
    for (int k = threadIdx.x; k < n; k += DL_BLOCK) acc += get(partials + k);
    const float sum = block_sum<DL_BLOCK>(acc, sh);
    if (threadIdx.x == 0) out[0] = sum / (float)P;
}

// v_pred = -(d term / d d) scale grad_out / (H W): sign(d) for L1 (sign(0) = 0), 2 d for L2.  min, max, median and the mean of gt carry
// no gradient (the reference takes the first two under no_grad; the others come from the data).
template <bool L2>
__global__ __launch_bounds__(DL_BLOCK) void depth_loss_bwd_kernel(int64_t P, const float* __restrict__ pred, const float* __restrict__ gt,
                                                                  DlNorm nm, DlMasks mk, const float* __restrict__ grad_out, float* __restrict__ v_pred) {
    const int64_t q = (int64_t)blockIdx.x * DL_BLOCK + threadIdx.x;
    if (q >= P) return;
    float gn, pn, scale;
    normalised_pair(nm, mk, q, pred[q], gt[q], gn, pn, scale);
    const float d = gn - pn, go = grad_out[0] / (float)P;
    const float dd = L2 ? 2.f * d : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
    v_pred[q] = -(dd * scale) * go;
}

int dl_partials(int64_t P) { return (int)((P + DL_PER_PARTIAL - 1) / DL_PER_PARTIAL); }

int check_depth_args(const char* who, int H, int W, int kind, int normalize, const void* pred, const void* gt) {
    if (H < 1 || W < 1 || (int64_t)H * W > DL_MAX) { set_error(who, "H and W must be >= 1 and H W <= 2^31"); return GSPL_ERR_INVALID_ARG; }
    if (kind != GSPL_DEPTH_LOSS_L1 && kind != GSPL_DEPTH_LOSS_L2) { set_error(who, "kind must be GSPL_DEPTH_LOSS_L1 or _L2 (l1+ssim is not built)"); return GSPL_ERR_UNSUPPORTED; }
    if (normalize < GSPL_DEPTH_NORM_NONE || normalize > GSPL_DEPTH_NORM_MEAN) return fail_arg(who);
    if (!pred || !gt) return fail_arg(who);
    return GSPL_OK;
}

}  // namespace
}  // namespace gspl

extern "C" size_t gspl_depth_loss_workspace_bytes(int H, int W) {
    if (H < 1 || W < 1 || (int64_t)H * W > gspl::DL_MAX) return 0;
    // 16 bytes of counters (what the memset clears) | stats [2] + padding | partials (two per workgroup for min / max)
    return 32 + 2 * sizeof(float) * (size_t)gspl::dl_partials((int64_t)H * W);
}

extern "C" int gspl_depth_loss_fwd(int H, int W, int kind, int normalize, const float* pred, const float* gt,
                                   const float* median, float median_value,
                                   const void* gt_mask, int gt_mask_u8, const void* pixel_mask, int pixel_mask_u8,
                                   void* workspace, size_t workspace_bytes, float* out, void* stream) {
    using namespace gspl;
    const char* who = "gspl_depth_loss_fwd";
    if (const int rc = check_depth_args(who, H, W, kind, normalize, pred, gt)) return rc;
    if (!workspace || !out || !aligned16(workspace)) return fail_arg(who);
    if (workspace_bytes < gspl_depth_loss_workspace_bytes(H, W)) return fail_ws(who);
    const int64_t P = (int64_t)H * W;
    const int n = dl_partials(P);
    hipStream_t s = (hipStream_t)stream;
    uint32_t* counters = (uint32_t*)workspace;
    float* stats = (float*)workspace + 4;
    float* partials = (float*)workspace + 8;
    if (const int rc = check_hip(hipMemsetAsync(workspace, 0, 16, s), who)) return rc;
    if (normalize == GSPL_DEPTH_NORM_MINMAX)
        hipLaunchKernelGGL(depth_stats_kernel<true>, dim3(n), dim3(DL_BLOCK), 0, s, P, pred, partials, counters, stats);
    else if (normalize == GSPL_DEPTH_NORM_MEAN)
        hipLaunchKernelGGL(depth_stats_kernel<false>, dim3(n), dim3(DL_BLOCK), 0, s, P, gt, partials, counters, stats);
    const DlNorm nm{normalize, stats, median, median_value};
    const DlMasks mk{gt_mask, pixel_mask, gt_mask_u8, pixel_mask_u8};
    dispatch_bools([&](auto l2) {
        hipLaunchKernelGGL(depth_loss_fwd_kernel<decltype(l2)::value>, dim3(n), dim3(DL_BLOCK), 0, s, P, pred, gt, nm, mk, partials, counters + 1, out);
    }, kind == GSPL_DEPTH_LOSS_L2);
    return check_launch(who);
}

extern "C" int gspl_depth_loss_bwd(int H, int W, int kind, int normalize, const float* pred, const float* gt,
                                   const float* median, float median_value,
                                   const void* gt_mask, int gt_mask_u8, const void* pixel_mask, int pixel_mask_u8,
                                   const void* workspace, const float* grad_out, float* v_pred, void* stream) {
    using namespace gspl;
    const char* who = "gspl_depth_loss_bwd";
    if (const int rc = check_depth_args(who, H, W, kind, normalize, pred, gt)) return rc;
    if (!workspace || !grad_out || !v_pred) return fail_arg(who);
    const int64_t P = (int64_t)H * W;
    const DlNorm nm{normalize, (const float*)workspace + 4, median, median_value};
    const DlMasks mk{gt_mask, pixel_mask, gt_mask_u8, pixel_mask_u8};
    dispatch_bools([&](auto l2) {
        hipLaunchKernelGGL(depth_loss_bwd_kernel<decltype(l2)::value>, dim3((unsigned)((P + DL_BLOCK - 1) / DL_BLOCK)), dim3(DL_BLOCK), 0, (hipStream_t)stream,
                           P, pred, gt, nm, mk, grad_out, v_pred);
    }, kind == GSPL_DEPTH_LOSS_L2);
    return check_launch(who);
}

// smooth.hip — local feature smoothing over a K-nearest-neighbour map, and the map's inverse adjacency (gfx950).
//
// Replaces the per-step smoothing of the SegAnyGS route (internal/segany_splatting.py:262-309):
//     n   = F.normalize(features, dim=-1)                      x / max(|x|, 1e-12)
//     m_i = mean over the selected columns k of n[idx[i, k]]    (the reference gathers an [N, S, D] tensor here)
//     out = m / (|m| + 1e-9)
// Forward: one launch, a group of lanes per row i gathers the S rows, normalises each on the fly (the row is in registers anyway)
// and writes out_i and |m_i|; the gather is never materialised.
// Backward: one launch, a group of lanes per row j.  The transpose of the gather is a walk over the INVERSE adjacency of the map —
// for row j the entries e = i * K + k with idx[i, k] == j, ascending (gspl_knn_graph) — filtered by the bit mask of the selected
// columns.  Per entry the group rebuilds dL/dm_i from v_out_i, out_i and |m_i|, adds it in list order, and finishes with the
// derivative of the first normalisation at x_j.  No atomics: the sum order is the list order, the same bits on every run.
//
// Lanes per row: 8 lanes x float4 when D is a multiple of 4, 32 lanes x 1 float otherwise; a lane holds up to 4 chunks (D <= 128).
#include <algorithm>
#include "gspl_device.h"
#include "gspl_host.h"
#include "gspl_sort.h"

namespace gspl {

static constexpr int SMOOTH_MAX_D = 128;
static constexpr int SMOOTH_MAX_K = 32;
static constexpr int SMOOTH_BLOCK = 256;
static constexpr int SMOOTH_CHUNKS = 4;      // chunks of VEC floats a lane holds: LPR * VEC * 4 >= 128

template <int VEC>
struct SmoothRow {
    float v[SMOOTH_CHUNKS][VEC];
};

template <int VEC, int LPR>
__device__ __forceinline__ void row_load(const float* __restrict__ p, int D, int lane, SmoothRow<VEC>& r) {
#pragma unroll
    for (int c = 0; c < SMOOTH_CHUNKS; ++c) {
        const int at = (c * LPR + lane) * VEC;
        if (at < D) {
            if constexpr (VEC == 4) {
                const float4 f = *reinterpret_cast<const float4*>(p + at);
                r.v[c][0] = f.x; r.v[c][1] = f.y; r.v[c][2] = f.z; r.v[c][3] = f.w;
            } else {
                r.v[c][0] = p[at];
            }
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) r.v[c][e] = 0.f;
        }
    }
}

template <int VEC, int LPR>
__device__ __forceinline__ void row_store(float* __restrict__ p, int D, int lane, const SmoothRow<VEC>& r) {
#pragma unroll
    for (int c = 0; c < SMOOTH_CHUNKS; ++c) {
        const int at = (c * LPR + lane) * VEC;
        if (at < D) {
            if constexpr (VEC == 4) *reinterpret_cast<float4*>(p + at) = make_float4(r.v[c][0], r.v[c][1], r.v[c][2], r.v[c][3]);
            else p[at] = r.v[c][0];
        }
    }
}

// sum over the LPR lanes of a row (LPR is a power of two and rows are aligned to it, so the partners are the row's own lanes)
template <int LPR>
__device__ __forceinline__ float row_sum(float x) {
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

template <int VEC, int LPR>
__device__ __forceinline__ float row_dot(const SmoothRow<VEC>& a, const SmoothRow<VEC>& b) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < SMOOTH_CHUNKS; ++c)
#pragma unroll
        for (int e = 0; e < VEC; ++e) s += a.v[c][e] * b.v[c][e];
    return row_sum<LPR>(s);
}

template <int VEC, int LPR>
__global__ __launch_bounds__(SMOOTH_BLOCK) void smooth_fwd_kernel(int N, int D, int K, uint32_t mask, float inv_s, const float* __restrict__ features,
                                                                  const int32_t* __restrict__ idx, float* __restrict__ out,
                                                                  float* __restrict__ mnorm) {
    const int lane = threadIdx.x % LPR;
    const int i = blockIdx.x * (SMOOTH_BLOCK / LPR) + threadIdx.x / LPR;
    if (i >= N) return;
    SmoothRow<VEC> acc, x;
#pragma unroll
    for (int c = 0; c < SMOOTH_CHUNKS; ++c)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc.v[c][e] = 0.f;
    for (int k = 0; k < K; ++k) {
        if (!((mask >> k) & 1u)) continue;
        const int j = idx[(size_t)i * K + k];
        row_load<VEC, LPR>(features + (size_t)j * D, D, lane, x);
        const float inv = 1.f / fmaxf(sqrtf(row_dot<VEC, LPR>(x, x)), 1e-12f);
#pragma unroll
        for (int c = 0; c < SMOOTH_CHUNKS; ++c)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc.v[c][e] += x.v[c][e] * inv;
    }
#pragma unroll
    for (int c = 0; c < SMOOTH_CHUNKS; ++c)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc.v[c][e] *= inv_s;
    const float r = sqrtf(row_dot<VEC, LPR>(acc, acc));
    const float scale = 1.f / (r + 1e-9f);
#pragma unroll
    for (int c = 0; c < SMOOTH_CHUNKS; ++c)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc.v[c][e] *= scale;
    row_store<VEC, LPR>(out + (size_t)i * D, D, lane, acc);
    if (lane == 0) mnorm[i] = r;
}

template <int VEC, int LPR>
__global__ __launch_bounds__(SMOOTH_BLOCK) void smooth_bwd_kernel(int N, int D, int K, uint32_t mask, float inv_s, const float* __restrict__ features,
                                                                  const uint32_t* __restrict__ row_start, const uint32_t* __restrict__ entries,
                                                                  const float* __restrict__ out, const float* __restrict__ mnorm,
                                                                  const float* __restrict__ v_out, float* __restrict__ v_features) {
    const int lane = threadIdx.x % LPR;
    const int j = blockIdx.x * (SMOOTH_BLOCK / LPR) + threadIdx.x / LPR;
    if (j >= N) return;
    SmoothRow<VEC> acc, g, o;
#pragma unroll
    for (int c = 0; c < SMOOTH_CHUNKS; ++c)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc.v[c][e] = 0.f;
    const uint32_t lo = row_start[j], hi = row_start[j + 1];
    for (uint32_t n = lo; n < hi; ++n) {
        const uint32_t entry = entries[n];
        const uint32_t i = entry / (uint32_t)K, k = entry - i * (uint32_t)K;
        if (!((mask >> k) & 1u)) continue;
        row_load<VEC, LPR>(v_out + (size_t)i * D, D, lane, g);
        row_load<VEC, LPR>(out + (size_t)i * D, D, lane, o);
        // out = m / (r + 1e-9), r = |m|:  dL/dm = g / (r + 1e-9) - out (g . out) / r   (the second term is d r, absent at r = 0)
        const float r = mnorm[i];
        const float a = 1.f / (r + 1e-9f);
        const float b = r > 0.f ? row_dot<VEC, LPR>(g, o) / r : 0.f;
#pragma unroll
        for (int c = 0; c < SMOOTH_CHUNKS; ++c)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc.v[c][e] += g.v[c][e] * a - o.v[c][e] * b;
    }
    // n = x / max(|x|, 1e-12): above the clamp dL/dx = (dn - n (n . dn)) / |x|, under it dL/dx = dn / 1e-12
    row_load<VEC, LPR>(features + (size_t)j * D, D, lane, o);
    const float norm = sqrtf(row_dot<VEC, LPR>(o, o));
    const bool clamped = !(norm >= 1e-12f);
    const float inv = 1.f / fmaxf(norm, 1e-12f);
    const float proj = clamped ? 0.f : row_dot<VEC, LPR>(o, acc) * inv_s * inv * inv;      // (n . dn) / |x|
#pragma unroll
    for (int c = 0; c < SMOOTH_CHUNKS; ++c)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc.v[c][e] = (acc.v[c][e] * inv_s - o.v[c][e] * proj) * inv;
    row_store<VEC, LPR>(v_features + (size_t)j * D, D, lane, acc);
}

// ---- inverse adjacency ------------------------------------------------------------------------------------------------------------
// keys[e] = idx[e] (N for an index outside 0 .. N-1, which sorts behind every row and is counted nowhere), vals[e] = e
__global__ __launch_bounds__(256) void graph_keys_kernel(uint32_t M, int N, const int32_t* __restrict__ idx, uint32_t* __restrict__ keys,
                                                         uint32_t* __restrict__ vals, uint32_t* __restrict__ count) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= M) return;
    const int32_t j = idx[e];
    const bool ok = j >= 0 && j < N;
    keys[e] = ok ? (uint32_t)j : (uint32_t)N;
    vals[e] = e;
    if (ok) atomicAdd(&count[j], 1u);
}

struct GraphWorkspace {
    RadixPlan plan;
    size_t keys0, keys1, vals_tmp, count, scan_tmp, sort_ws, total;
};

static bool plan_graph(int N, int K, GraphWorkspace& w) {
    const size_t M = (size_t)N * (size_t)K;
    if (N < 0 || K < 1 || K > SMOOTH_MAX_K || M > RADIX_MAX_ITEMS) return false;
    int bits = 1;
    while (((uint64_t)1 << bits) <= (uint64_t)N) ++bits;      // the keys are 0 .. N
    if (!radix_plan(M, 0, bits, 8, RADIX_TILE_U32, w.plan)) return false;
    const size_t m = M > 0 ? M : 1;
    Carve c;
    w.keys0 = c.take(4 * m);
    w.keys1 = c.take(4 * m);
    w.vals_tmp = c.take(4 * m);
    w.count = c.take(4 * ((size_t)N + 1));
    w.scan_tmp = c.take(exclusive_scan_u32_workspace_bytes((size_t)N + 1));
    w.sort_ws = c.take(w.plan.total_bytes ? w.plan.total_bytes : 16);
    w.total = c.off;
    return true;
}

template <int VEC, int LPR>
static void smooth_launch(bool fwd, int N, int D, int K, uint32_t mask, float inv_s, const float* features, const int32_t* idx,
                          const uint32_t* row_start, const uint32_t* entries, float* out, float* mnorm, const float* v_out, float* v_features,
                          hipStream_t s) {
    const int rows = SMOOTH_BLOCK / LPR;
    const dim3 grid((N + rows - 1) / rows), block(SMOOTH_BLOCK);
    if (fwd) hipLaunchKernelGGL((smooth_fwd_kernel<VEC, LPR>), grid, block, 0, s, N, D, K, mask, inv_s, features, idx, out, mnorm);
    else hipLaunchKernelGGL((smooth_bwd_kernel<VEC, LPR>), grid, block, 0, s, N, D, K, mask, inv_s, features, row_start, entries,
                            (const float*)out, (const float*)mnorm, v_out, v_features);
}

static int smooth_args(int N, int D, int K, uint32_t mask, const char* who) {
    if (N < 0 || D < 1 || D > SMOOTH_MAX_D || K < 1 || K > SMOOTH_MAX_K) return fail_arg(who);
    const uint32_t all = K == 32 ? 0xFFFFFFFFu : ((1u << K) - 1u);
    if (mask == 0 || (mask & ~all)) return fail_arg(who);
    return GSPL_OK;
}

}  // namespace gspl

extern "C" size_t gspl_knn_graph_workspace_bytes(int N, int K) {
    gspl::GraphWorkspace w;
    return gspl::plan_graph(N, K, w) ? w.total : 0;
}

extern "C" int gspl_knn_graph(int N, int K, const int32_t* idx, uint32_t* row_start, uint32_t* entries, void* workspace, size_t workspace_bytes,
                              void* stream) {
    using namespace gspl;
    GraphWorkspace w;
    if (!plan_graph(N, K, w)) return fail_arg("knn_graph: bad size (1 <= K <= 32, N * K < 2^30)");
    if (!row_start) return fail_arg("knn_graph: NULL required pointer");
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) return check_hip(hipMemsetAsync(row_start, 0, 4, s), "knn_graph: memset");
    if (!idx || !entries || !workspace) return fail_arg("knn_graph: NULL required pointer");
    if (workspace_bytes < w.total) return fail_ws("knn_graph");
    char* ws = (char*)workspace;
    const uint32_t M = (uint32_t)((size_t)N * K);
    uint32_t* count = (uint32_t*)(ws + w.count);
    // the stable sort leaves its result in buffer (passes & 1): that one is `entries`
    const int res = w.plan.passes & 1;
    uint32_t* keys[2] = {(uint32_t*)(ws + w.keys0), (uint32_t*)(ws + w.keys1)};
    uint32_t* vals[2];
    vals[res] = entries;
    vals[1 - res] = (uint32_t*)(ws + w.vals_tmp);
    hipError_t e = hipMemsetAsync(count, 0, 4 * ((size_t)N + 1), s);
    if (e != hipSuccess) return check_hip(e, "knn_graph: memset");
    hipLaunchKernelGGL(graph_keys_kernel, dim3((M + 255u) / 256u), dim3(256), 0, s, M, N, idx, keys[0], vals[0], count);
    int rc = check_launch("knn_graph: keys");
    if (rc != GSPL_OK) return rc;
    rc = exclusive_scan_u32((const uint32_t*)count, row_start, (size_t)N + 1, ws + w.scan_tmp, s);
    if (rc != GSPL_OK) return rc;
    return radix_sort_u32(w.plan, ws + w.sort_ws, keys, vals, false, s);
}

extern "C" int gspl_smooth_features_fwd(int N, int D, int K, uint32_t mask, const float* features, const int32_t* idx, float* out, float* mnorm,
                                        void* stream) {
    using namespace gspl;
    int rc = smooth_args(N, D, K, mask, "smooth_features_fwd: bad size or column mask (1 <= D <= 128, 1 <= K <= 32)");
    if (rc != GSPL_OK || N == 0) return rc;
    if (!features || !idx || !out || !mnorm) return fail_arg("smooth_features_fwd: NULL required pointer");
    const float inv_s = 1.f / (float)__builtin_popcount(mask);
    if (D % 4 == 0 && aligned16(features) && aligned16(out))
        smooth_launch<4, 8>(true, N, D, K, mask, inv_s, features, idx, nullptr, nullptr, out, mnorm, nullptr, nullptr, (hipStream_t)stream);
    else
        smooth_launch<1, 32>(true, N, D, K, mask, inv_s, features, idx, nullptr, nullptr, out, mnorm, nullptr, nullptr, (hipStream_t)stream);
    return check_launch("smooth_features_fwd");
}

extern "C" int gspl_smooth_features_bwd(int N, int D, int K, uint32_t mask, const float* features, const uint32_t* row_start, const uint32_t* entries,
                                        const float* out, const float* mnorm, const float* v_out, float* v_features, void* stream) {
    using namespace gspl;
    int rc = smooth_args(N, D, K, mask, "smooth_features_bwd: bad size or column mask (1 <= D <= 128, 1 <= K <= 32)");
    if (rc != GSPL_OK || N == 0) return rc;
    if (!features || !row_start || !entries || !out || !mnorm || !v_out || !v_features) return fail_arg("smooth_features_bwd: NULL required pointer");
    const float inv_s = 1.f / (float)__builtin_popcount(mask);
    if (D % 4 == 0 && aligned16(features) && aligned16(out) && aligned16(v_out) && aligned16(v_features))
        smooth_launch<4, 8>(false, N, D, K, mask, inv_s, features, nullptr, row_start, entries, (float*)out, (float*)mnorm, v_out, v_features,
                            (hipStream_t)stream);
    else
        smooth_launch<1, 32>(false, N, D, K, mask, inv_s, features, nullptr, row_start, entries, (float*)out, (float*)mnorm, v_out, v_features,
                             (hipStream_t)stream);
    return check_launch("smooth_features_bwd");
}

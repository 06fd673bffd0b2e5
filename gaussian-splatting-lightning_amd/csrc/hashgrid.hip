// hashgrid.hip — multiresolution hash-grid / dense-grid encoding with linear interpolation, forward and backward (gfx950).
//
// What `tinycudann.Encoding` with otype HashGrid / DenseGrid computes (the SWAG route: internal/models/swag_model.py:75-78); the
// rules are those of include/gspl_hip.h section 20.  The level table (scale, resolution, first row, row count of each level) is
// computed by the caller on the host and travels to the kernels BY VALUE in the kernel arguments: a level is one blockIdx.y, so
// every read of the table is a scalar load with a wave-uniform index.
//
// Forward: one lane per (point, level); the 2^D rows of F floats are vector loads, the F outputs one vector store.
// Backward, table: F lanes per (point, level), one float per lane, so that one wave-instruction adds 64 / F whole rows of 4 F
//   bytes (not 64 single floats in 64 rows).  A (point, level) whose F values of v_out are all zero adds nothing and a wave of such
//   points returns before it reads x.  Before each atomic the lanes of a wave that hold the SAME destination row in consecutive
//   points are summed (a segmented scan over run numbers, skipped by a ballot when no two neighbours agree): points that arrive
//   in a spatially coherent order, and every point at the coarse dense levels of a clustered cloud, then share one add.
// Backward, x (optional): one lane per point walks the levels; no atomics, the same bits on every run.
#include <cstdint>
#include "gspl_host.h"

namespace gspl {

static constexpr int HG_MAX_LEVELS = 32;
static constexpr int HG_BLOCK = 256;

struct HgLevels {
    float scale[HG_MAX_LEVELS];
    uint32_t res[HG_MAX_LEVELS];
    uint32_t size[HG_MAX_LEVELS];        // rows of the level
    uint32_t first[HG_MAX_LEVELS];       // first row of the level
    uint32_t hashed;                     // bit l: level l is hashed
};

template <int F> struct HgRow { float v[F]; };

template <int F>
__device__ __forceinline__ HgRow<F> hg_load(const float* __restrict__ p) {
    HgRow<F> r;
    if constexpr (F == 1) {
        r.v[0] = p[0];
    } else if constexpr (F == 2) {
        const float2 a = *reinterpret_cast<const float2*>(p);
        r.v[0] = a.x; r.v[1] = a.y;
    } else {
#pragma unroll
        for (int c = 0; c < F / 4; ++c) {
            const float4 a = reinterpret_cast<const float4*>(p)[c];
            r.v[4 * c] = a.x; r.v[4 * c + 1] = a.y; r.v[4 * c + 2] = a.z; r.v[4 * c + 3] = a.w;
        }
    }
    return r;
}

template <int F>
__device__ __forceinline__ void hg_store(float* __restrict__ p, const HgRow<F>& r) {
    if constexpr (F == 1) {
        p[0] = r.v[0];
    } else if constexpr (F == 2) {
        *reinterpret_cast<float2*>(p) = make_float2(r.v[0], r.v[1]);
    } else {
#pragma unroll
        for (int c = 0; c < F / 4; ++c)
            reinterpret_cast<float4*>(p)[c] = make_float4(r.v[4 * c], r.v[4 * c + 1], r.v[4 * c + 2], r.v[4 * c + 3]);
    }
}

// pos = fma(x, scale, 0.5): ONE rounding; cell = floor(pos) through int32 to uint32 (negative cells wrap); frac = pos - cell (exact)
template <int D>
struct HgPos {
    uint32_t cell[D];
    float frac[D];
};

template <int D>
__device__ __forceinline__ HgPos<D> hg_position(const float* __restrict__ x, float scale) {
    HgPos<D> p;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float pos = __fmaf_rn(x[d], scale, 0.5f);
        const float fl = floorf(pos);
        p.cell[d] = (uint32_t)(int32_t)fl;
        p.frac[d] = pos - fl;
    }
    return p;
}

// row of a corner inside its level: dense sum c_d res^d, or the XOR of c_d prime_d, in uint32; then mod the level's row count
template <int D>
__device__ __forceinline__ uint32_t hg_row(const HgPos<D>& p, int corner, uint32_t res, uint32_t size, bool hashed) {
    constexpr uint32_t primes[3] = {1u, 2654435761u, 805459861u};
    uint32_t dense = 0, hash = 0, stride = 1;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const uint32_t c = p.cell[d] + ((corner >> d) & 1);
        dense += c * stride;
        stride *= res;
        hash ^= c * primes[d];
    }
    const uint32_t at = hashed ? hash : dense;
    return (size & (size - 1)) == 0 ? at & (size - 1) : at % size;      // (wave-uniform: a level's row count)
}

template <int D>
__device__ __forceinline__ float hg_weight(const HgPos<D>& p, int corner) {
    float w = 1.f;
#pragma unroll
    for (int d = 0; d < D; ++d) w *= ((corner >> d) & 1) ? p.frac[d] : 1.f - p.frac[d];
    return w;
}

template <int D, int F>
__global__ __launch_bounds__(HG_BLOCK) void hashgrid_fwd_kernel(int N, int L, HgLevels lv, const float* __restrict__ x,
                                                                const float* __restrict__ table, float* __restrict__ out) {
    const int l = blockIdx.y;
    const int n = blockIdx.x * HG_BLOCK + threadIdx.x;
    if (n >= N) return;
    const uint32_t res = lv.res[l], size = lv.size[l];
    const bool hashed = (lv.hashed >> l) & 1u;
    const float* __restrict__ rows = table + (size_t)lv.first[l] * F;
    const HgPos<D> p = hg_position<D>(x + (size_t)n * D, lv.scale[l]);
    HgRow<F> acc;
#pragma unroll
    for (int f = 0; f < F; ++f) acc.v[f] = 0.f;
#pragma unroll
    for (int c = 0; c < (1 << D); ++c) {
        const uint32_t row = hg_row<D>(p, c, res, size, hashed);
        const float w = hg_weight<D>(p, c);
        const HgRow<F> t = hg_load<F>(rows + (size_t)row * F);
#pragma unroll
        for (int f = 0; f < F; ++f) acc.v[f] = fmaf(w, t.v[f], acc.v[f]);
    }
    hg_store<F>(out + ((size_t)n * L + l) * F, acc);
}

template <int D, int F>
__global__ __launch_bounds__(HG_BLOCK) void hashgrid_bwd_table_kernel(int N, int L, HgLevels lv, const float* __restrict__ x,
                                                                      const float* __restrict__ v_out, float* __restrict__ v_table) {
    constexpr int PTS = 64 / F;                    // points of a wave
    const int l = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int f = threadIdx.x % F;
    const int n = blockIdx.x * (HG_BLOCK / F) + threadIdx.x / F;
    const bool valid = n < N;
    const float g = valid ? v_out[((size_t)n * L + l) * F + f] : 0.f;
    // a point takes part when one of its F values is not zero
    const unsigned long long nonzero = __ballot(g != 0.f);
    const bool active = ((nonzero >> (lane & ~(F - 1))) & ((1ull << F) - 1)) != 0;
    if (nonzero == 0) return;                      // the whole wave: no shuffle or barrier follows for it
    const uint32_t res = lv.res[l], size = lv.size[l];
    const bool hashed = (lv.hashed >> l) & 1u;
    float* __restrict__ rows = v_table + (size_t)lv.first[l] * F;
    float xs[D];
#pragma unroll
    for (int d = 0; d < D; ++d) xs[d] = valid ? x[(size_t)n * D + d] : 0.f;
    const HgPos<D> p = hg_position<D>(xs, lv.scale[l]);
    const unsigned long long group_end = (lane | (F - 1)) == 63 ? ~0ull : ((2ull << (lane | (F - 1))) - 1);
#pragma unroll
    for (int c = 0; c < (1 << D); ++c) {
        // a point that does not take part gets a key no row has (size <= 2^31)
        const uint32_t key = active ? hg_row<D>(p, c, res, size, hashed) : 0xffffffffu;
        float val = hg_weight<D>(p, c) * g;
        const uint32_t key_before = __shfl_up(key, F, 64);
        const bool head = lane < F || key_before != key;
        const unsigned long long heads = __ballot(head);
        if (__ballot(!head && active) != 0) {
            // consecutive points with one destination form a run; its last point adds the run's sum
            const int run = __popcll(heads & group_end);
#pragma unroll
            for (int d = 1; d < PTS; d *= 2) {
                const float val_before = __shfl_up(val, d * F, 64);
                const int run_there = __shfl_up(run, d * F, 64);
                if (lane >= d * F && run_there == run) val += val_before;
            }
        }
        const bool last = lane + F >= 64 || ((heads >> (lane + F)) & 1ull);
        if (active && last) atomicAdd(rows + (size_t)key * F + f, val);
    }
}

template <int D, int F>
__global__ __launch_bounds__(HG_BLOCK) void hashgrid_bwd_x_kernel(int N, int L, HgLevels lv, const float* __restrict__ x,
                                                                  const float* __restrict__ table, const float* __restrict__ v_out,
                                                                  float* __restrict__ v_x) {
    const int n = blockIdx.x * HG_BLOCK + threadIdx.x;
    if (n >= N) return;
    float acc[D];
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = 0.f;
    for (int l = 0; l < L; ++l) {
        const HgRow<F> g = hg_load<F>(v_out + ((size_t)n * L + l) * F);
        bool any = false;
#pragma unroll
        for (int f = 0; f < F; ++f) any = any || g.v[f] != 0.f;
        if (!any) continue;
        const uint32_t res = lv.res[l], size = lv.size[l];
        const bool hashed = (lv.hashed >> l) & 1u;
        const float scale = lv.scale[l];
        const float* __restrict__ rows = table + (size_t)lv.first[l] * F;
        const HgPos<D> p = hg_position<D>(x + (size_t)n * D, scale);
        float level[D];
#pragma unroll
        for (int d = 0; d < D; ++d) level[d] = 0.f;
#pragma unroll
        for (int c = 0; c < (1 << D); ++c) {
            const HgRow<F> t = hg_load<F>(rows + (size_t)hg_row<D>(p, c, res, size, hashed) * F);
            float dot = 0.f;
#pragma unroll
            for (int f = 0; f < F; ++f) dot = fmaf(t.v[f], g.v[f], dot);
#pragma unroll
            for (int d = 0; d < D; ++d) {
                float w = ((c >> d) & 1) ? 1.f : -1.f;
#pragma unroll
                for (int e = 0; e < D; ++e)
                    if (e != d) w *= ((c >> e) & 1) ? p.frac[e] : 1.f - p.frac[e];
                level[d] = fmaf(w, dot, level[d]);
            }
        }
#pragma unroll
        for (int d = 0; d < D; ++d) acc[d] = fmaf(scale, level[d], acc[d]);
    }
#pragma unroll
    for (int d = 0; d < D; ++d) v_x[(size_t)n * D + d] = acc[d];
}

// f(std::integral_constant<int, D>, std::integral_constant<int, F>) for the built (D, F); the caller has checked both
template <class Fn>
static int hg_dispatch(int D, int F, Fn&& fn) {
    return dispatch_int<2, 3>(D, [&](auto d) { return dispatch_int<1, 2, 4, 8>(F, [&](auto f) { return fn(d, f); }); });
}

// The argument checks both entries share; fills `lv`.  scales, resolutions [L] and offsets [L + 1] are HOST arrays.
static int hg_levels(const char* who, int N, int D, int F, int L, const float* scales, const uint32_t* resolutions, const uint32_t* offsets,
                     HgLevels& lv) {
    if (N < 0) return fail_arg(who);
    if (D != 2 && D != 3) { set_error(who, "n_input_dims must be 2 or 3"); return GSPL_ERR_INVALID_ARG; }
    if (F != 1 && F != 2 && F != 4 && F != 8) { set_error(who, "n_features_per_level must be 1, 2, 4 or 8"); return GSPL_ERR_INVALID_ARG; }
    if (L < 1 || L > HG_MAX_LEVELS) { set_error(who, "n_levels must be 1 .. 32"); return GSPL_ERR_INVALID_ARG; }
    if (!scales || !resolutions || !offsets) return fail_arg(who);
    lv.hashed = 0;
    for (int l = 0; l < L; ++l) {
        if (offsets[l + 1] <= offsets[l] || resolutions[l] < 1) { set_error(who, "every level needs at least one row and a resolution"); return GSPL_ERR_INVALID_ARG; }
        const uint32_t size = offsets[l + 1] - offsets[l];
        if (size > 0x80000000u) { set_error(who, "a level has at most 2^31 rows"); return GSPL_ERR_INVALID_ARG; }
        uint64_t cells = 1;
        for (int d = 0; d < D; ++d) cells = cells * resolutions[l] > (1ull << 40) ? (1ull << 40) : cells * resolutions[l];
        lv.scale[l] = scales[l];
        lv.res[l] = resolutions[l];
        lv.size[l] = size;
        lv.first[l] = offsets[l];
        if (cells > size) lv.hashed |= 1u << l;
    }
    for (int l = L; l < HG_MAX_LEVELS; ++l) { lv.scale[l] = 0.f; lv.res[l] = 1; lv.size[l] = 1; lv.first[l] = 0; }
    return GSPL_OK;
}

static bool hg_aligned(const void* p, int F) { return ((uintptr_t)p % (size_t)(F >= 4 ? 16 : 4 * F)) == 0; }

}  // namespace gspl

using namespace gspl;

extern "C" int gspl_hashgrid_fwd(int N, int D, int F, int L, const float* scales, const uint32_t* resolutions, const uint32_t* offsets,
                                 const float* x, const float* table, float* out, void* stream) {
    HgLevels lv;
    if (const int rc = hg_levels("gspl_hashgrid_fwd", N, D, F, L, scales, resolutions, offsets, lv)) return rc;
    if (N == 0) return GSPL_OK;
    if (!x || !table || !out) return fail_arg("gspl_hashgrid_fwd");
    if (!hg_aligned(table, F) || !hg_aligned(out, F)) { set_error("gspl_hashgrid_fwd", "table and out must be aligned to a row of F floats (16 bytes from F = 4)"); return GSPL_ERR_INVALID_ARG; }
    const dim3 grid((N + HG_BLOCK - 1) / HG_BLOCK, L);
    return hg_dispatch(D, F, [&](auto d, auto f) {
        hipLaunchKernelGGL((hashgrid_fwd_kernel<decltype(d)::value, decltype(f)::value>), grid, dim3(HG_BLOCK), 0, (hipStream_t)stream, N, L, lv, x, table, out);
        return check_launch("gspl_hashgrid_fwd");
    });
}

extern "C" int gspl_hashgrid_bwd(int N, int D, int F, int L, const float* scales, const uint32_t* resolutions, const uint32_t* offsets,
                                 const float* x, const float* table, const float* v_out, float* v_table, float* v_x, void* stream) {
    HgLevels lv;
    if (const int rc = hg_levels("gspl_hashgrid_bwd", N, D, F, L, scales, resolutions, offsets, lv)) return rc;
    if (N == 0) return GSPL_OK;
    if (!x || !v_out || (!v_table && !v_x) || (v_x && !table)) return fail_arg("gspl_hashgrid_bwd");
    if (!hg_aligned(v_out, F) || (v_x && !hg_aligned(table, F))) { set_error("gspl_hashgrid_bwd", "table and v_out must be aligned to a row of F floats (16 bytes from F = 4)"); return GSPL_ERR_INVALID_ARG; }
    return hg_dispatch(D, F, [&](auto d, auto f) {
        if (v_table) {
            const int points = HG_BLOCK / decltype(f)::value;
            hipLaunchKernelGGL((hashgrid_bwd_table_kernel<decltype(d)::value, decltype(f)::value>), dim3((N + points - 1) / points, L), dim3(HG_BLOCK), 0, (hipStream_t)stream,
                               N, L, lv, x, v_out, v_table);
            if (const int rc = check_launch("gspl_hashgrid_bwd (table)")) return rc;
        }
        if (v_x) {
            hipLaunchKernelGGL((hashgrid_bwd_x_kernel<decltype(d)::value, decltype(f)::value>), dim3((N + HG_BLOCK - 1) / HG_BLOCK), dim3(HG_BLOCK), 0, (hipStream_t)stream,
                               N, L, lv, x, table, v_out, v_x);
            return check_launch("gspl_hashgrid_bwd (x)");
        }
        return (int)GSPL_OK;
    });
}

// taming.hip — the scoring arithmetic of the Taming-3DGS density controller (gfx950; include/gspl_hip.h section 27).
//
// Restates internal/density_controllers/taming_3dgs_density_controller.py: `Taming3DGSUtils.normalize` (:455-465) and the aggregate of
// `compute_gaussian_score` (:536-553), and `get_edges` (:367-373) with the min-max normalisation of `on_train_start` (:138).
//
//   positive medians   the median of the entries > 0 of up to 16 rows, by an EXACT radix select on the bit pattern (positive floats
//                      order like their bits): three digit passes of 11 + 11 + 9 bits.  A pass is one launch over all rows (grid.y = row):
//                      integer atomics into an LDS histogram per workgroup, its nonzero bins flushed by integer atomics into the row's
//                      global counters; then a launch of one workgroup per row scans the counters and fixes the digit that holds the rank.
//                      Plain launches in stream order: no "last workgroup" counter, no spinning, no float atomics, nothing read by the host.
//                      Every pass reads each row once, front to back: 4 R N bytes, the traffic of a contiguous copy's source side.
//   score accumulate   one launch per view, 9 rows in and one row in / out: HBM-bound, 4 (R + 1) + 1 bytes read and 4 written per Gaussian.
//   edge map           PIL's `convert('L')` and `ImageFilter.FIND_EDGES` in integers, e / 255, then (x - min) / (max - min): the filter
//                      with a min / max per workgroup, then the normalisation, which first folds those.
//
// Contraction is OFF: every operation of the score and of the normalisation is rounded on its own, as the reference's torch ops are
// (the error counts of tests/test_taming_gpu.py are per operation).
#pragma clang fp contract(off)
#include "gspl_device.h"
#include "gspl_host.h"

namespace gspl {

static constexpr int TAMING_BLOCK = 256;
static constexpr int TAMING_PER_THREAD = 16;                                   // elements per thread and workgroup, in fours
static constexpr int TAMING_CHUNK = TAMING_BLOCK * TAMING_PER_THREAD;          // 4096 elements per workgroup
static constexpr int MEDIAN_BINS = GSPL_TAMING_MEDIAN_BINS;                    // 2048: the widest digit (11 bits)
static constexpr int MEDIAN_PASSES = 3;
// digit p of a key: (key >> SHIFT) & (2^BITS - 1) with SHIFT 20, 9, 0 and BITS 11, 11, 9: the keys of valid entries have bit 31 clear

struct TamingRows {                       // by value in the kernel arguments: no table in device memory
    const void* p[GSPL_TAMING_MAX_ROWS];
    int is_i32[GSPL_TAMING_MAX_ROWS];     // 1: int32 entries, read as float(x)
};
struct TamingCoeffs { float c[GSPL_TAMING_MAX_ROWS]; };
// what a select launch leaves for the next pass, per row
struct MedianState { uint32_t prefix; uint32_t rank; uint32_t n; uint32_t pad; };

// The bit pattern an entry is ranked by (an int32 entry through float(x): x <= 0 gives a pattern that is not valid).
__device__ __forceinline__ uint32_t taming_key(uint32_t raw, int is_i32) {
    return is_i32 ? __float_as_uint((float)(int32_t)raw) : raw;
}
// > 0 and not NaN, on the bits: sign clear, non-zero, at most +inf.  No comparison of floats: subnormals count whatever the flush mode.
__device__ __forceinline__ bool taming_valid(uint32_t key) { return key - 1u < 0x7f800000u; }

// four entries from element i on (i a multiple of 4): one 16-byte load where the row allows it; entries past N come back as 0 (not valid)
__device__ __forceinline__ void taming_load4(const uint32_t* __restrict__ row, bool vec, int64_t i, int64_t N, uint32_t v[4]) {
    if (vec && i + 3 < N) {
        const uint4 q = *reinterpret_cast<const uint4*>(row + i);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (i + k < N) ? row[i + k] : 0u;
    }
}

// One digit pass over all rows.  grid = (ceil(N / 4096), R).  state: the previous select's (not read in pass 0).  hist [R][2048] of THIS pass.
template <int PASS>
__global__ __launch_bounds__(TAMING_BLOCK) void median_hist_kernel(TamingRows rows, int64_t N, const MedianState* __restrict__ state,
                                                                  uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[MEDIAN_BINS];
    const int tid = threadIdx.x, r = blockIdx.y, lane = tid & 63;
    constexpr int SHIFT = PASS == 0 ? 20 : (PASS == 1 ? 9 : 0);
    constexpr int BITS = PASS == 2 ? 9 : 11;
    constexpr int ABOVE = SHIFT + BITS;                      // the bits above this digit are the prefix (pass 0: bit 31, clear when valid)
    for (int b = tid; b < (1 << BITS); b += TAMING_BLOCK) h[b] = 0u;
    uint32_t prefix = 0u;
    if (PASS > 0) {
        const MedianState st = state[r];
        if (st.n == 0u) return;                              // no valid entry in this row: nothing to count (uniform over the workgroup)
        prefix = st.prefix >> ABOVE;
    }
    __syncthreads();
    const uint32_t* __restrict__ row = reinterpret_cast<const uint32_t*>(rows.p[r]);
    const int is_i32 = rows.is_i32[r];
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15u) == 0;
    const int64_t base = (int64_t)blockIdx.x * TAMING_CHUNK;
#pragma unroll 1
    for (int it = 0; it < TAMING_PER_THREAD / 4; ++it) {
        const int64_t i = base + (int64_t)it * (TAMING_BLOCK * 4) + (int64_t)tid * 4;
        if (base + (int64_t)it * (TAMING_BLOCK * 4) >= N) break;         // uniform over the workgroup
        uint32_t v[4];
        taming_load4(row, vec, i, N, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t key = taming_key(v[k], is_i32);
            const bool on = taming_valid(key) && (PASS == 0 || (key >> ABOVE) == prefix);
            const uint32_t digit = (key >> SHIFT) & ((1u << BITS) - 1u);
            // a wave whose counted entries all fall into one bin (a row inside one binade in pass 0; any row late in the select) adds once
            const unsigned long long votes = __ballot(on);
            if (votes == 0ull) continue;
            const uint32_t d0 = __shfl(digit, __ffsll((long long)votes) - 1, 64);
            const unsigned long long same = __ballot(on && digit == d0);
            if (same == votes) {
                if (lane == __ffsll((long long)votes) - 1) atomicAdd(&h[d0], (uint32_t)__popcll(votes));
            } else if (on) {
                atomicAdd(&h[digit], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t* __restrict__ out = hist + (size_t)r * MEDIAN_BINS;
    for (int b = tid; b < (1 << BITS); b += TAMING_BLOCK) {
        const uint32_t c = h[b];
        if (c) atomicAdd(&out[b], c);
    }
}

// One workgroup per row: the bin of this pass's counters that holds the rank.  Pass 0 also fixes n and the rank (n - 1) / 2; the last
// pass writes the count and the median (NaN when n == 0).
template <int PASS>
__global__ __launch_bounds__(TAMING_BLOCK) void median_select_kernel(const uint32_t* __restrict__ hist, MedianState* __restrict__ state,
                                                                    int32_t* __restrict__ counts, float* __restrict__ medians) {
    __shared__ uint32_t s_wave[TAMING_BLOCK / 64];
    const int tid = threadIdx.x, r = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int SHIFT = PASS == 0 ? 20 : (PASS == 1 ? 9 : 0);
    constexpr int PER = MEDIAN_BINS / TAMING_BLOCK;          // 8 bins per thread, contiguous (the bins a pass does not use hold 0)
    const uint32_t* __restrict__ hr = hist + (size_t)r * MEDIAN_BINS;
    MedianState st = MedianState{0u, 0u, 0u, 0u};
    if (PASS > 0) st = state[r];                             // read by every thread BEFORE the barrier; one thread writes it after
    uint32_t c[PER], mine = 0u;
#pragma unroll
    for (int k = 0; k < PER; ++k) { c[k] = hr[tid * PER + k]; mine += c[k]; }
    uint32_t incl = mine;                                    // inclusive scan over the workgroup, in thread order
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(incl, off, 64);
        if (lane >= off) incl += y;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
#pragma unroll
    for (int w = 0; w < TAMING_BLOCK / 64; ++w) {
        if (w < wave) before += s_wave[w];
        total += s_wave[w];
    }
    uint32_t n, rank, prefix;
    if (PASS == 0) { n = total; rank = n ? (n - 1u) / 2u : 0u; prefix = 0u; }
    else { n = st.n; rank = st.rank; prefix = st.prefix; }
    if (n == 0u) {
        if (tid == 0) {
            if (PASS == 0) state[r] = MedianState{0u, 0u, 0u, 0u};
            if (PASS == MEDIAN_PASSES - 1) { counts[r] = 0; medians[r] = __uint_as_float(0x7fc00000u); }
        }
        return;
    }
    uint32_t lo = before + incl - mine;                      // entries in the bins before this thread's
    if (rank >= lo && rank < lo + mine) {                    // exactly one thread: the counters of a pass sum to the entries it ranked
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (rank < lo + c[k]) {
                const uint32_t p = prefix | ((uint32_t)(tid * PER + k) << SHIFT);
                if (PASS == MEDIAN_PASSES - 1) { counts[r] = (int32_t)n; medians[r] = __uint_as_float(p); }
                else state[r] = MedianState{p, rank - lo, n, 0u};
                break;
            }
            lo += c[k];
        }
    }
}

// importance[g] += ((w * (p + q)) * visible[g]),  q = the first n_first rows' terms added left to right, p = the others', a term being
// c_r * (v_r[g] / median_r) where v_r[g] is valid and 0 where it is not (the reference's association, :536-553).
__global__ __launch_bounds__(TAMING_BLOCK) void taming_score_kernel(TamingRows rows, TamingCoeffs coeffs, int R, int n_first, int64_t N,
                                                                   const int32_t* __restrict__ counts, const float* __restrict__ medians,
                                                                   const float* __restrict__ w, const uint8_t* __restrict__ visible,
                                                                   float* __restrict__ importance) {
    __shared__ float s_med[GSPL_TAMING_MAX_ROWS];
    __shared__ int s_on[GSPL_TAMING_MAX_ROWS];               // a row without a valid entry (n = 0, median NaN) contributes nothing
    if (threadIdx.x < GSPL_TAMING_MAX_ROWS) {
        const bool on = threadIdx.x < R && counts[threadIdx.x] > 0;
        s_on[threadIdx.x] = on ? 1 : 0;
        s_med[threadIdx.x] = on ? medians[threadIdx.x] : 1.f;
    }
    __syncthreads();
    const float wv = w[0];
    for (int64_t g = (int64_t)blockIdx.x * TAMING_BLOCK + threadIdx.x; g < N; g += (int64_t)gridDim.x * TAMING_BLOCK) {
        float first = 0.f, rest = 0.f;
        for (int r = 0; r < R; ++r) {
            const uint32_t raw = reinterpret_cast<const uint32_t*>(rows.p[r])[g];
            const uint32_t key = taming_key(raw, rows.is_i32[r]);
            const float term = (s_on[r] && taming_valid(key)) ? coeffs.c[r] * (__uint_as_float(key) / s_med[r]) : 0.f;
            if (r == 0) first = term;
            else if (r < n_first) first = first + term;
            else if (r == n_first) rest = term;
            else rest = rest + term;
        }
        const float sum = n_first < R ? rest + first : first;
        const float agg = (wv * sum) * (visible[g] ? 1.f : 0.f);
        importance[g] = importance[g] + agg;
    }
}

// PIL's L conversion of a pixel: bytes straight from a uint8 image, floats as ToPILImage quantises them (x * 255 truncated; NaN and
// what lies outside [0, 255] after the product clamp, which the reference leaves undefined)
template <bool FLOAT>
__device__ __forceinline__ int taming_grey(const void* __restrict__ image, int64_t plane, int64_t i) {
    int c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (FLOAT) {
            const float x = reinterpret_cast<const float*>(image)[k * plane + i] * 255.f;
            c[k] = x >= 255.f ? 255 : (x > 0.f ? (int)x : 0);
        } else {
            c[k] = reinterpret_cast<const uint8_t*>(image)[k * plane + i];
        }
    }
    return (c[0] * 19595 + c[1] * 38470 + c[2] * 7471 + 0x8000) >> 16;
}

static constexpr int EDGE_PER_THREAD = 16;
static constexpr int EDGE_CHUNK = TAMING_BLOCK * EDGE_PER_THREAD;

// FIND_EDGES (3x3, -1 with centre 8, clipped to 0 .. 255; the one-pixel border is the grey image) -> out = e / 255, and the workgroup's
// smallest and largest e into partial[2 b], partial[2 b + 1]
template <bool FLOAT>
__global__ __launch_bounds__(TAMING_BLOCK) void edges_filter_kernel(const void* __restrict__ image, int H, int W, float* __restrict__ out,
                                                                   int32_t* __restrict__ partial) {
    __shared__ int s_lo[TAMING_BLOCK / 64], s_hi[TAMING_BLOCK / 64];
    const int64_t plane = (int64_t)H * W;
    const int64_t base = (int64_t)blockIdx.x * EDGE_CHUNK;
    int lo = 255, hi = 0;
    for (int k = 0; k < EDGE_PER_THREAD; ++k) {
        const int64_t i = base + (int64_t)k * TAMING_BLOCK + threadIdx.x;
        if (i >= plane) break;
        const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
        int e = taming_grey<FLOAT>(image, plane, i);
        if (y > 0 && y < H - 1 && x > 0 && x < W - 1) {
            int around = 0;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx)
                    if (dy != 0 || dx != 0) around += taming_grey<FLOAT>(image, plane, i + (int64_t)dy * W + dx);
            e = min(max(8 * e - around, 0), 255);
        }
        out[i] = (float)e / 255.f;
        lo = min(lo, e);
        hi = max(hi, e);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off, 64));
        hi = max(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < TAMING_BLOCK / 64; ++w) { lo = min(lo, s_lo[w]); hi = max(hi, s_hi[w]); }
        partial[2 * (int64_t)blockIdx.x] = lo;
        partial[2 * (int64_t)blockIdx.x + 1] = hi;
    }
}

// out = (out - min) / (max - min), min and max folded from the n_partial pairs first (integers: the order does not matter); a constant
// EDGE image (a black frame, a constant one without an interior) divides 0 by 0 and is NaN throughout, as in the reference
__global__ __launch_bounds__(TAMING_BLOCK) void edges_normalise_kernel(int64_t plane, const int32_t* __restrict__ partial, int n_partial,
                                                                      float* __restrict__ out) {
    __shared__ int s_lo[TAMING_BLOCK / 64], s_hi[TAMING_BLOCK / 64];
    int lo = 255, hi = 0;
    for (int b = threadIdx.x; b < n_partial; b += TAMING_BLOCK) {
        lo = min(lo, partial[2 * (int64_t)b]);
        hi = max(hi, partial[2 * (int64_t)b + 1]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off, 64));
        hi = max(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    for (int w = 0; w < TAMING_BLOCK / 64; ++w) { lo = min(lo, s_lo[w]); hi = max(hi, s_hi[w]); }
    const float fmin = (float)lo / 255.f, fmax = (float)hi / 255.f;
    const float range = fmax - fmin;
    const int64_t base = (int64_t)blockIdx.x * EDGE_CHUNK;
    for (int k = 0; k < EDGE_PER_THREAD; ++k) {
        const int64_t i = base + (int64_t)k * TAMING_BLOCK + threadIdx.x;
        if (i >= plane) break;
        out[i] = (out[i] - fmin) / range;
    }
}

static bool taming_rows(int R, const void* const* rows, const int32_t* is_i32, TamingRows& t) {
    for (int r = 0; r < GSPL_TAMING_MAX_ROWS; ++r) {
        if (r < R && (!rows[r] || (reinterpret_cast<uintptr_t>(rows[r]) & 3u))) return false;
        t.p[r] = r < R ? rows[r] : nullptr;
        t.is_i32[r] = (r < R && is_i32[r]) ? 1 : 0;
    }
    return true;
}

}  // namespace gspl

extern "C" size_t gspl_positive_medians_workspace_bytes(int R) {
    using namespace gspl;
    if (R < 1 || R > GSPL_TAMING_MAX_ROWS) return 0;
    return up256((size_t)MEDIAN_PASSES * R * MEDIAN_BINS * sizeof(uint32_t)) + up256((size_t)R * sizeof(MedianState));
}

extern "C" int gspl_positive_medians(int R, int64_t N, const void* const* rows, const int32_t* is_i32, int32_t* counts, float* medians,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    using namespace gspl;
    if (R < 1 || R > GSPL_TAMING_MAX_ROWS || N < 1 || N > 0x7fffffffll) return fail_arg("positive_medians: R must be 1 .. 16 and N 1 .. 2^31 - 1");
    if (!rows || !is_i32 || !counts || !medians || !workspace) return fail_arg("positive_medians: NULL required pointer");
    TamingRows t;
    if (!taming_rows(R, rows, is_i32, t)) return fail_arg("positive_medians: a row pointer is NULL or not aligned to 4 bytes");
    if (workspace_bytes < gspl_positive_medians_workspace_bytes(R)) return fail_ws("positive_medians");
    hipStream_t s = (hipStream_t)stream;
    const size_t hist_bytes = (size_t)MEDIAN_PASSES * R * MEDIAN_BINS * sizeof(uint32_t);
    uint32_t* hist = reinterpret_cast<uint32_t*>(workspace);
    MedianState* state = reinterpret_cast<MedianState*>(reinterpret_cast<char*>(workspace) + up256(hist_bytes));
    if (int rc = check_hip(hipMemsetAsync(hist, 0, hist_bytes, s), "positive_medians: clearing the counters")) return rc;
    const dim3 grid((unsigned)((N + TAMING_CHUNK - 1) / TAMING_CHUNK), (unsigned)R), block(TAMING_BLOCK);
    uint32_t* h0 = hist;
    uint32_t* h1 = hist + (size_t)R * MEDIAN_BINS;
    uint32_t* h2 = hist + (size_t)2 * R * MEDIAN_BINS;
    hipLaunchKernelGGL(median_hist_kernel<0>, grid, block, 0, s, t, N, (const MedianState*)state, h0);
    hipLaunchKernelGGL(median_select_kernel<0>, dim3(R), block, 0, s, (const uint32_t*)h0, state, counts, medians);
    hipLaunchKernelGGL(median_hist_kernel<1>, grid, block, 0, s, t, N, (const MedianState*)state, h1);
    hipLaunchKernelGGL(median_select_kernel<1>, dim3(R), block, 0, s, (const uint32_t*)h1, state, counts, medians);
    hipLaunchKernelGGL(median_hist_kernel<2>, grid, block, 0, s, t, N, (const MedianState*)state, h2);
    hipLaunchKernelGGL(median_select_kernel<2>, dim3(R), block, 0, s, (const uint32_t*)h2, state, counts, medians);
    return check_launch("positive_medians");
}

extern "C" int gspl_taming_score_accumulate(int R, int n_first, int64_t N, const void* const* rows, const int32_t* is_i32,
                                            const float* coeffs, const int32_t* counts, const float* medians, const float* w,
                                            const uint8_t* visible, float* importance, void* stream) {
    using namespace gspl;
    if (R < 1 || R > GSPL_TAMING_MAX_ROWS || n_first < 1 || n_first > R || N < 0 || N > 0x7fffffffll)
        return fail_arg("taming_score_accumulate: R must be 1 .. 16, n_first 1 .. R and N 0 .. 2^31 - 1");
    if (N == 0) return GSPL_OK;
    if (!rows || !is_i32 || !coeffs || !counts || !medians || !w || !visible || !importance)
        return fail_arg("taming_score_accumulate: NULL required pointer");
    TamingRows t;
    if (!taming_rows(R, rows, is_i32, t)) return fail_arg("taming_score_accumulate: a row pointer is NULL or not aligned to 4 bytes");
    TamingCoeffs c;
    for (int r = 0; r < GSPL_TAMING_MAX_ROWS; ++r) c.c[r] = r < R ? coeffs[r] : 0.f;
    const int64_t blocks = (N + TAMING_BLOCK - 1) / TAMING_BLOCK;
    hipLaunchKernelGGL(taming_score_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(TAMING_BLOCK), 0, (hipStream_t)stream, t, c, R,
                       n_first, N, counts, medians, w, visible, importance);
    return check_launch("taming_score_accumulate");
}

extern "C" int gspl_find_edges_partials(int H, int W) {
    if (H < 1 || W < 1 || (int64_t)H * W > 0x7fffffffll) return 0;
    return (int)(((int64_t)H * W + gspl::EDGE_CHUNK - 1) / gspl::EDGE_CHUNK);
}

extern "C" int gspl_find_edges(int H, int W, const void* image, int is_float, float* out, int32_t* partial, int n_partial, void* stream) {
    using namespace gspl;
    const int blocks = gspl_find_edges_partials(H, W);
    if (blocks == 0) return fail_arg("find_edges: H and W must be >= 1 and H W <= 2^31 - 1");
    if (!image || !out || !partial) return fail_arg("find_edges: NULL required pointer");
    if (n_partial < blocks) return fail_ws("find_edges");
    hipStream_t s = (hipStream_t)stream;
    if (is_float) hipLaunchKernelGGL(edges_filter_kernel<true>, dim3(blocks), dim3(TAMING_BLOCK), 0, s, image, H, W, out, partial);
    else hipLaunchKernelGGL(edges_filter_kernel<false>, dim3(blocks), dim3(TAMING_BLOCK), 0, s, image, H, W, out, partial);
    hipLaunchKernelGGL(edges_normalise_kernel, dim3(blocks), dim3(TAMING_BLOCK), 0, s, (int64_t)H * W, (const int32_t*)partial, blocks, out);
    return check_launch("find_edges");
}

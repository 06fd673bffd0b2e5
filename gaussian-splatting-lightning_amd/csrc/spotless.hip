// spotless.hip — the SpotLessSplats route outside the rasterizer (gfx950): the mask predictor with its backward, the per-pixel error
// with its histogram and robust masks, and the masked L1 loss.  The rules are those of include/gspl_hip.h section 23.
//
// What `SpotLessMetricsModule.mlp_mask` of the reference computes (internal/metrics/spotless_metrics.py) after the fold of its first
// linear layer through the bilinear resampling:
//     z[i, j, :] = bilinear(G)[i, j, :] + A[i, :] + B[j, :];   mask[i, j] = sigmoid(w2 . relu(z) + b2)
// G [h0, w0, 16] is channel-last: a corner is one 64-byte row, read through the caches (the table is 160 KB at 50 x 50 and every
// neighbouring pixel shares its corners).
//
// Forward: one lane per output pixel; with a second resampling the network is evaluated at the four source pixels of the output pixel
//   and the mask itself is never written.
// Backward: no float atomics, every sum in a fixed order.
//   sls_bwd_rows_kernel, one wave per (64 mask columns, row y of G): walks the mask rows whose upper corner row is y - 1 or y, one
//     column per lane.  It recomputes z, forms dz, and keeps per lane T[y, j, :] = sum_i wy(i, y) dz[i, j, :] (the row half of the
//     adjoint bilinear).  Of the rows it OWNS (upper corner row == y; every mask row has exactly one owner) it also keeps the column
//     sums, the sums for w2 and b2, and writes the row sum of its 64 columns (a fixed butterfly).
//   sls_bwd_final_kernel: v_G = the column half of the adjoint over T, v_B = sum over y of the column sums, v_A = sum over the column
//     blocks, v_w2 | v_b2 = one wave per value over the (y, block) partials.
//   A pixel whose incoming gradient is zero is not evaluated; a wave of such pixels only writes its zeros.
//
// Both resamplings follow F.interpolate(mode="bilinear", align_corners=False): sls_axis, the source index by one fused multiply-add as
// torch's own kernels compute it (pinned against F.interpolate's weights in tests/test_spotless_cpu.py), nothing else contracted.
#include <cstdint>
#include "gspl_host.h"
#include "gspl_reduce.h"
#include "gspl_resample.h"

namespace gspl {
namespace {

constexpr int SLS_HID = 16;            // hidden units (the reference's Linear(.., 16))
constexpr int SLS_BLOCK = 256;
constexpr int SLS_MAX_DIM = 16384;     // every map, mask and image dimension: sls_range's float estimate is then off by far less than 1
constexpr int SLS_MAX_BINS = 15360;    // 60 KB of LDS for the private histogram

// SlsAxis and sls_axis (the rule of one resampled axis) are in gspl_resample.h, shared with segany.hip.

// the weight with which output o reads source s
__device__ __forceinline__ float sls_weight(const SlsAxis& a, int s) { return (a.i0 == s ? a.h : 0.f) + (a.i1 == s ? a.l : 0.f); }

// [lo, hi]: a range of outputs that holds every o whose i0 is s - 1 or s (the only outputs that read source s); the exact test is
// sls_weight.  i0 is monotone in o, the estimate is off by far less than the margin of 2 for dimensions up to SLS_MAX_DIM.
__device__ __forceinline__ void sls_range(float scale, int s, int O, int& lo, int& hi) {
    const float inv = 1.f / scale;
    lo = max((int)floorf(((float)s - 0.5f) * inv - 0.5f) - 2, 0);
    hi = min((int)ceilf(((float)s + 1.5f) * inv - 0.5f) + 2, O - 1);
}

struct SlsShape {
    int h0, w0, mh, mw, H, W;            // H == 0: no second resampling, the output is the mask
    float sy, sx, ry, rx;                // (float)h0 / mh, w0 / mw;  mh / H, mw / W
};

struct SlsHead { float w2[SLS_HID], b2; };

__device__ __forceinline__ SlsHead sls_head(const float* __restrict__ w2, const float* __restrict__ b2) {
    SlsHead hd;
#pragma unroll
    for (int c = 0; c < SLS_HID; ++c) hd.w2[c] = w2[c];
    hd.b2 = b2[0];
    return hd;
}

// z of mask pixel (i, j): the bilinear sample of G (the two columns of a row first, then the two rows), then + A[i], then + B[j]
__device__ __forceinline__ void sls_hidden(const SlsShape& p, const float* __restrict__ G, const float* __restrict__ A, const float* __restrict__ B,
                                           int i, int j, float z[SLS_HID]) {
    const SlsAxis y = sls_axis(p.sy, i, p.h0), x = sls_axis(p.sx, j, p.w0);
    const float4* g00 = reinterpret_cast<const float4*>(G + ((size_t)y.i0 * p.w0 + x.i0) * SLS_HID);
    const float4* g01 = reinterpret_cast<const float4*>(G + ((size_t)y.i0 * p.w0 + x.i1) * SLS_HID);
    const float4* g10 = reinterpret_cast<const float4*>(G + ((size_t)y.i1 * p.w0 + x.i0) * SLS_HID);
    const float4* g11 = reinterpret_cast<const float4*>(G + ((size_t)y.i1 * p.w0 + x.i1) * SLS_HID);
    const float4* a = reinterpret_cast<const float4*>(A + (size_t)i * SLS_HID);
    const float4* b = reinterpret_cast<const float4*>(B + (size_t)j * SLS_HID);
#pragma unroll
    for (int q = 0; q < SLS_HID / 4; ++q) {
        const float4 v00 = g00[q], v01 = g01[q], v10 = g10[q], v11 = g11[q], va = a[q], vb = b[q];
        const float t00[4] = {v00.x, v00.y, v00.z, v00.w}, t01[4] = {v01.x, v01.y, v01.z, v01.w};
        const float t10[4] = {v10.x, v10.y, v10.z, v10.w}, t11[4] = {v11.x, v11.y, v11.z, v11.w};
        const float ta[4] = {va.x, va.y, va.z, va.w}, tb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float top = fmaf(x.l, t01[k], x.h * t00[k]);
            const float bot = fmaf(x.l, t11[k], x.h * t10[k]);
            const float v = fmaf(y.l, bot, y.h * top);
            z[4 * q + k] = (v + ta[k]) + tb[k];
        }
    }
}

// y = b2 + sum_c w2[c] relu(z[c]) as one fmaf chain from c = 0
__device__ __forceinline__ float sls_pre(const SlsHead& hd, const float z[SLS_HID]) {
    float acc = hd.b2;
#pragma unroll
    for (int c = 0; c < SLS_HID; ++c) acc = fmaf(hd.w2[c], fmaxf(z[c], 0.f), acc);
    return acc;
}

__device__ __forceinline__ float sls_sigmoid(float y) { return 1.f / (1.f + expf(-y)); }

// s (1 - s) = e / (1 + e)^2 with e = exp(-|y|): no cancellation where the sigmoid saturates
__device__ __forceinline__ float sls_sigmoid_slope(float y) {
    const float e = expf(-fabsf(y)), d = 1.f + e;
    return e / (d * d);
}

__device__ __forceinline__ float sls_mask_at(const SlsShape& p, const SlsHead& hd, const float* __restrict__ G, const float* __restrict__ A,
                                             const float* __restrict__ B, int i, int j) {
    float z[SLS_HID];
    sls_hidden(p, G, A, B, i, j, z);
    return sls_sigmoid(sls_pre(hd, z));
}

template <bool RESAMPLE>
__global__ __launch_bounds__(SLS_BLOCK) void sls_fwd_kernel(SlsShape p, const float* __restrict__ G, const float* __restrict__ A,
                                                            const float* __restrict__ B, const float* __restrict__ w2, const float* __restrict__ b2,
                                                            float* __restrict__ out) {
    const int OW = RESAMPLE ? p.W : p.mw, OH = RESAMPLE ? p.H : p.mh;
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * (SLS_BLOCK / 64) + (threadIdx.x >> 6);
    if (ox >= OW || oy >= OH) return;
    const SlsHead hd = sls_head(w2, b2);
    float s;
    if (RESAMPLE) {
        const SlsAxis y = sls_axis(p.ry, oy, p.mh), x = sls_axis(p.rx, ox, p.mw);
        const float m00 = sls_mask_at(p, hd, G, A, B, y.i0, x.i0), m01 = sls_mask_at(p, hd, G, A, B, y.i0, x.i1);
        const float m10 = sls_mask_at(p, hd, G, A, B, y.i1, x.i0), m11 = sls_mask_at(p, hd, G, A, B, y.i1, x.i1);
        const float top = fmaf(x.l, m01, x.h * m00), bot = fmaf(x.l, m11, x.h * m10);
        s = fmaf(y.l, bot, y.h * top);
    } else {
        s = sls_mask_at(p, hd, G, A, B, oy, ox);
    }
    out[(size_t)oy * OW + ox] = s;
}

// the gradient that reaches mask pixel (i, j): v_out itself, or the adjoint of the second resampling gathered in a fixed order
template <bool RESAMPLE>
__device__ __forceinline__ float sls_incoming(const SlsShape& p, const float* __restrict__ v_out, int i, int j) {
    if (!RESAMPLE) return v_out[(size_t)i * p.mw + j];
    int ylo, yhi, xlo, xhi;
    sls_range(p.ry, i, p.H, ylo, yhi);
    sls_range(p.rx, j, p.W, xlo, xhi);
    float v = 0.f;
    for (int oy = ylo; oy <= yhi; ++oy) {
        const float wy = sls_weight(sls_axis(p.ry, oy, p.mh), i);
        if (wy == 0.f) continue;
        float row = 0.f;
        for (int ox = xlo; ox <= xhi; ++ox) {
            const float wx = sls_weight(sls_axis(p.rx, ox, p.mw), j);
            if (wx != 0.f) row = fmaf(wx, v_out[(size_t)oy * p.W + ox], row);
        }
        v = fmaf(wy, row, v);
    }
    return v;
}

// Partials, all [.., 16] rows but pw: pt [h0, mw] (T), pb [h0, mw] (owned column sums), pa [mh, ncb] (row sums per column block),
// pw [h0, ncb, 17] (w2's sixteen sums, then b2's)
template <bool RESAMPLE>
__global__ __launch_bounds__(64) void sls_bwd_rows_kernel(SlsShape p, int ncb, const float* __restrict__ G, const float* __restrict__ A,
                                                          const float* __restrict__ B, const float* __restrict__ w2, const float* __restrict__ b2,
                                                          const float* __restrict__ v_out, float* __restrict__ pt, float* __restrict__ pb,
                                                          float* __restrict__ pa, float* __restrict__ pw) {
    const int cb = blockIdx.x, y = blockIdx.y, lane = threadIdx.x;
    const int j = cb * 64 + lane;
    const bool valid = j < p.mw;
    const SlsHead hd = sls_head(w2, b2);
    float T[SLS_HID], col[SLS_HID], sw[SLS_HID], sb = 0.f;
#pragma unroll
    for (int c = 0; c < SLS_HID; ++c) T[c] = col[c] = sw[c] = 0.f;
    int lo, hi;
    sls_range(p.sy, y, p.mh, lo, hi);
    for (int i = lo; i <= hi; ++i) {
        const SlsAxis ay = sls_axis(p.sy, i, p.h0);
        const float wy = sls_weight(ay, y);
        const bool owned = ay.i0 == y;
        if (!owned && wy == 0.f) continue;                 // (the same for every lane)
        const float v = valid ? sls_incoming<RESAMPLE>(p, v_out, i, j) : 0.f;
        float dz[SLS_HID];
#pragma unroll
        for (int c = 0; c < SLS_HID; ++c) dz[c] = 0.f;
        const bool live = v != 0.f;
        if (live) {
            float z[SLS_HID];
            sls_hidden(p, G, A, B, i, j, z);
            const float dy = v * sls_sigmoid_slope(sls_pre(hd, z));
#pragma unroll
            for (int c = 0; c < SLS_HID; ++c) {
                dz[c] = z[c] > 0.f ? dy * hd.w2[c] : 0.f;
                T[c] = fmaf(wy, dz[c], T[c]);
                if (owned) {
                    col[c] += dz[c];
                    sw[c] = fmaf(dy, fmaxf(z[c], 0.f), sw[c]);
                }
            }
            if (owned) sb += dy;
        }
        if (owned) {
            float* row = pa + ((size_t)i * ncb + cb) * SLS_HID;
            if (__ballot(live) == 0) {
                if (lane < SLS_HID) row[lane] = 0.f;
            } else {
#pragma unroll
                for (int c = 0; c < SLS_HID; ++c) {
                    const float sum = wave_sum(dz[c]);
                    if (lane == c) row[c] = sum;
                }
            }
        }
    }
    if (valid) {
        float4* t4 = reinterpret_cast<float4*>(pt + ((size_t)y * p.mw + j) * SLS_HID);
        float4* b4 = reinterpret_cast<float4*>(pb + ((size_t)y * p.mw + j) * SLS_HID);
#pragma unroll
        for (int q = 0; q < SLS_HID / 4; ++q) {
            t4[q] = make_float4(T[4 * q], T[4 * q + 1], T[4 * q + 2], T[4 * q + 3]);
            b4[q] = make_float4(col[4 * q], col[4 * q + 1], col[4 * q + 2], col[4 * q + 3]);
        }
    }
    float* w = pw + ((size_t)y * ncb + cb) * (SLS_HID + 1);
#pragma unroll
    for (int c = 0; c < SLS_HID; ++c) {
        const float sum = wave_sum(sw[c]);
        if (lane == c) w[c] = sum;
    }
    const float sum = wave_sum(sb);
    if (lane == SLS_HID) w[SLS_HID] = sum;
}

// One flat index space: [0, 17 * 64) one wave per value of v_w2 | v_b2, then one lane per value of v_G, v_B, v_A
__global__ __launch_bounds__(SLS_BLOCK) void sls_bwd_final_kernel(SlsShape p, int ncb, const float* __restrict__ pt, const float* __restrict__ pb,
                                                                  const float* __restrict__ pa, const float* __restrict__ pw,
                                                                  float* __restrict__ v_G, float* __restrict__ v_A, float* __restrict__ v_B,
                                                                  float* __restrict__ v_w) {
    constexpr int NW = (SLS_HID + 1) * 64;
    const int64_t t = (int64_t)blockIdx.x * SLS_BLOCK + threadIdx.x;
    if (t < NW) {
        const int k = (int)t >> 6, lane = (int)t & 63, n = p.h0 * ncb;
        float acc = 0.f;
        for (int r = lane; r < n; r += 64) acc += pw[(size_t)r * (SLS_HID + 1) + k];
        acc = wave_sum(acc);
        if (lane == 0) v_w[k] = acc;
        return;
    }
    int64_t u = t - NW;
    const int64_t nG = (int64_t)p.h0 * p.w0 * SLS_HID, nB = (int64_t)p.mw * SLS_HID, nA = (int64_t)p.mh * SLS_HID;
    if (u < nG) {
        const int c = (int)(u % SLS_HID), x = (int)((u / SLS_HID) % p.w0), y = (int)(u / ((int64_t)SLS_HID * p.w0));
        int lo, hi;
        sls_range(p.sx, x, p.mw, lo, hi);
        float acc = 0.f;
        for (int j = lo; j <= hi; ++j) {
            const float wx = sls_weight(sls_axis(p.sx, j, p.w0), x);
            if (wx != 0.f) acc = fmaf(wx, pt[((size_t)y * p.mw + j) * SLS_HID + c], acc);
        }
        v_G[u] = acc;
        return;
    }
    u -= nG;
    if (u < nB) {
        float acc = 0.f;
        for (int y = 0; y < p.h0; ++y) acc += pb[(size_t)y * p.mw * SLS_HID + u];
        v_B[u] = acc;
        return;
    }
    u -= nB;
    if (u < nA) {
        const int c = (int)(u % SLS_HID);
        const int64_t i = u / SLS_HID;
        float acc = 0.f;
        for (int cb = 0; cb < ncb; ++cb) acc += pa[((size_t)i * ncb + cb) * SLS_HID + c];
        v_A[u] = acc;
    }
}

// ---- the per-pixel error, its histogram and the two robust masks -------------------------------------------------------------------
constexpr int SLS_TILE = 16;
constexpr int SLS_HALO = SLS_TILE + 2;

// One workgroup walks tiles of 16 x 16 pixels with a stride of the grid; its histogram lives in LDS (integer atomics) and only the
// bins it touched go to memory at the end.
__global__ __launch_bounds__(SLS_BLOCK) void sls_error_stats_kernel(int H, int W, int bins, int tiles_x, int n_tiles, const float* __restrict__ render,
                                                                    const float* __restrict__ gt, const float* __restrict__ thresholds,
                                                                    const float* __restrict__ edges, float* __restrict__ err, int32_t* __restrict__ counts,
                                                                    float* __restrict__ lower_mask, float* __restrict__ upper_mask) {
    extern __shared__ int32_t sls_hist[];
    __shared__ uint8_t inl[SLS_HALO][SLS_HALO];            // bit 0: below the lower threshold, bit 1: below the upper
    for (int k = threadIdx.x; k < bins; k += SLS_BLOCK) sls_hist[k] = 0;
    const float lower = thresholds[0], upper = thresholds[1];
    const size_t P = (size_t)H * W;
    const int tx = threadIdx.x % SLS_TILE, ty = threadIdx.x / SLS_TILE;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int x0 = (tile % tiles_x) * SLS_TILE, y0 = (tile / tiles_x) * SLS_TILE;
        __syncthreads();                                   // the histogram is clear / the last tile's flags are read
        for (int k = threadIdx.x; k < SLS_HALO * SLS_HALO; k += SLS_BLOCK) {
            const int hy = k / SLS_HALO, hx = k % SLS_HALO;
            const int y = y0 + hy - 1, x = x0 + hx - 1;
            uint8_t flags = 0;                             // outside the image: no inlier (zero padding)
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const size_t at = (size_t)y * W + x;
                const float d0 = fabsf(render[at] - gt[at]), d1 = fabsf(render[P + at] - gt[P + at]), d2 = fabsf(render[2 * P + at] - gt[2 * P + at]);
                const float e = ((d0 + d1) + d2) / 3.f;
                flags = (e < lower ? 1 : 0) | (e < upper ? 2 : 0);
                if (hy >= 1 && hy <= SLS_TILE && hx >= 1 && hx <= SLS_TILE) {      // the tile's own pixel: written and counted once
                    err[at] = e;
                    if (e >= 0.f && e <= 1.f) {
                        // torch.histogram: the bin from the position, then the search among the neighbouring edges
                        const int pos = (int)(e * (float)bins);
                        int k0 = max(pos - 1, 0);
                        const int k1 = min(pos + 2, bins + 1);
                        while (k0 < k1 && !(e < edges[k0])) ++k0;      // the first edge above e
                        atomicAdd(&sls_hist[min(max(k0 - 1, 0), bins - 1)], 1);      // (the last bin includes 1)
                    }
                }
            }
            inl[hy][hx] = flags;
        }
        __syncthreads();
        const int y = y0 + ty, x = x0 + tx;
        if (y < H && x < W) {
            int n_lower = 0, n_upper = 0;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int f = inl[ty + dy][tx + dx];
                    n_lower += f & 1;
                    n_upper += f >> 1;
                }
            }
            const int own = inl[ty + 1][tx + 1];
            lower_mask[(size_t)y * W + x] = ((own & 1) || n_lower >= 5) ? 1.f : 0.f;
            upper_mask[(size_t)y * W + x] = ((own & 2) || n_upper >= 5) ? 1.f : 0.f;
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < bins; k += SLS_BLOCK) {
        const int32_t n = sls_hist[k];
        if (n) atomicAdd(&counts[k], n);
    }
}

// ---- the masked L1 ---------------------------------------------------------------------------------------------------------------------
constexpr int SLS_L1_CHAIN = 8;                            // pixels per lane of a partial
constexpr int SLS_L1_PER_PARTIAL = SLS_BLOCK * SLS_L1_CHAIN;
// (block_sum of gspl_reduce.h: lanes by butterfly, then the four waves in order; thread 0 gets the sum)

__global__ __launch_bounds__(SLS_BLOCK) void sls_l1_partials_kernel(int64_t P, const float* __restrict__ render, const float* __restrict__ gt,
                                                                    const float* __restrict__ mask, float* __restrict__ partials) {
    __shared__ float sh[SLS_BLOCK / 64];
    const int64_t base = (int64_t)blockIdx.x * SLS_L1_PER_PARTIAL + threadIdx.x;
    float acc = 0.f;
    for (int k = 0; k < SLS_L1_CHAIN; ++k) {
        const int64_t q = base + (int64_t)k * SLS_BLOCK;
        if (q >= P) break;
        const float d = (fabsf(render[q] - gt[q]) + fabsf(render[P + q] - gt[P + q])) + fabsf(render[2 * P + q] - gt[2 * P + q]);
        acc = fmaf(mask[q], d, acc);
    }
    const float total = block_sum<SLS_BLOCK>(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(SLS_BLOCK) void sls_l1_final_kernel(int n_partials, float denom, const float* __restrict__ partials, float* __restrict__ out) {
    __shared__ float sh[SLS_BLOCK / 64];
    float acc = 0.f;
    for (int k = threadIdx.x; k < n_partials; k += SLS_BLOCK) acc += partials[k];
    const float total = block_sum<SLS_BLOCK>(acc, sh);
    if (threadIdx.x == 0) out[0] = total / denom;
}

__global__ __launch_bounds__(SLS_BLOCK) void sls_l1_bwd_kernel(int64_t P, double denom, const float* __restrict__ render, const float* __restrict__ gt,
                                                               const float* __restrict__ mask, const float* __restrict__ grad_out,
                                                               float* __restrict__ v_render) {
    const int64_t q = (int64_t)blockIdx.x * SLS_BLOCK + threadIdx.x;
    if (q >= P) return;
    const float g = (float)(((double)grad_out[0] / denom) * (double)mask[q]);      // rounded to float32 once
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float d = render[c * P + q] - gt[c * P + q];
        v_render[c * P + q] = d > 0.f ? g : (d < 0.f ? -g : 0.f);
    }
}

bool sls_dim(int n) { return n >= 2 && n <= SLS_MAX_DIM; }

int sls_shape(const char* who, int h0, int w0, int mh, int mw, int H, int W, SlsShape& p) {
    if (!sls_dim(h0) || !sls_dim(w0) || !sls_dim(mh) || !sls_dim(mw)) { set_error(who, "every map and mask dimension must be 2 .. 16384"); return GSPL_ERR_INVALID_ARG; }
    if ((H == 0) != (W == 0) || (H != 0 && (!sls_dim(H) || !sls_dim(W)))) { set_error(who, "H and W must both be 0 (no second resampling) or 2 .. 16384"); return GSPL_ERR_INVALID_ARG; }
    p = SlsShape{h0, w0, mh, mw, H, W, (float)h0 / (float)mh, (float)w0 / (float)mw, H ? (float)mh / (float)H : 1.f, W ? (float)mw / (float)W : 1.f};
    return GSPL_OK;
}

int sls_blocks(int mw) { return (mw + 63) / 64; }

struct SlsPartials { size_t pt, pb, pa, pw, total; };
SlsPartials sls_partials(int h0, int mh, int mw) {
    const size_t ncb = (size_t)sls_blocks(mw);
    Carve c;
    SlsPartials s;
    s.pt = c.take((size_t)h0 * mw * SLS_HID * sizeof(float));
    s.pb = c.take((size_t)h0 * mw * SLS_HID * sizeof(float));
    s.pa = c.take((size_t)mh * ncb * SLS_HID * sizeof(float));
    s.pw = c.take((size_t)h0 * ncb * (SLS_HID + 1) * sizeof(float));
    s.total = c.off;
    return s;
}

}  // namespace
}  // namespace gspl

using namespace gspl;

extern "C" int gspl_spotless_mask_fwd(int h0, int w0, int mh, int mw, int H, int W, const float* G, const float* A, const float* B,
                                      const float* w2, const float* b2, float* out, void* stream) {
    SlsShape p;
    if (const int rc = sls_shape("gspl_spotless_mask_fwd", h0, w0, mh, mw, H, W, p)) return rc;
    if (!G || !A || !B || !w2 || !b2 || !out) return fail_arg("gspl_spotless_mask_fwd");
    if (!aligned16(G) || !aligned16(A) || !aligned16(B)) { set_error("gspl_spotless_mask_fwd", "G, A and B must be aligned to 16 bytes"); return GSPL_ERR_INVALID_ARG; }
    const int OH = H ? H : mh, OW = W ? W : mw;
    const dim3 grid((OW + 63) / 64, (OH + SLS_BLOCK / 64 - 1) / (SLS_BLOCK / 64));
    if (H) hipLaunchKernelGGL(sls_fwd_kernel<true>, grid, dim3(SLS_BLOCK), 0, (hipStream_t)stream, p, G, A, B, w2, b2, out);
    else hipLaunchKernelGGL(sls_fwd_kernel<false>, grid, dim3(SLS_BLOCK), 0, (hipStream_t)stream, p, G, A, B, w2, b2, out);
    return check_launch("gspl_spotless_mask_fwd");
}

extern "C" size_t gspl_spotless_mask_workspace_bytes(int h0, int w0, int mh, int mw) {
    if (!sls_dim(h0) || !sls_dim(w0) || !sls_dim(mh) || !sls_dim(mw)) return 0;
    return sls_partials(h0, mh, mw).total;
}

extern "C" int gspl_spotless_mask_bwd(int h0, int w0, int mh, int mw, int H, int W, const float* G, const float* A, const float* B,
                                      const float* w2, const float* b2, const float* v_out, float* v_G, float* v_A, float* v_B, float* v_w,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    SlsShape p;
    if (const int rc = sls_shape("gspl_spotless_mask_bwd", h0, w0, mh, mw, H, W, p)) return rc;
    if (!G || !A || !B || !w2 || !b2 || !v_out || !v_G || !v_A || !v_B || !v_w || !workspace) return fail_arg("gspl_spotless_mask_bwd");
    if (!aligned16(G) || !aligned16(A) || !aligned16(B) || !aligned16(workspace)) {
        set_error("gspl_spotless_mask_bwd", "G, A, B and the workspace must be aligned to 16 bytes");
        return GSPL_ERR_INVALID_ARG;
    }
    const SlsPartials s = sls_partials(h0, mh, mw);
    if (workspace_bytes < s.total) return fail_ws("gspl_spotless_mask_bwd");
    char* ws = (char*)workspace;
    float *pt = (float*)(ws + s.pt), *pb = (float*)(ws + s.pb), *pa = (float*)(ws + s.pa), *pw = (float*)(ws + s.pw);
    const int ncb = sls_blocks(mw);
    const dim3 grid(ncb, h0);
    if (H) hipLaunchKernelGGL(sls_bwd_rows_kernel<true>, grid, dim3(64), 0, (hipStream_t)stream, p, ncb, G, A, B, w2, b2, v_out, pt, pb, pa, pw);
    else hipLaunchKernelGGL(sls_bwd_rows_kernel<false>, grid, dim3(64), 0, (hipStream_t)stream, p, ncb, G, A, B, w2, b2, v_out, pt, pb, pa, pw);
    if (const int rc = check_launch("gspl_spotless_mask_bwd (rows)")) return rc;
    const int64_t n = (int64_t)(SLS_HID + 1) * 64 + ((int64_t)h0 * w0 + mw + mh) * SLS_HID;
    hipLaunchKernelGGL(sls_bwd_final_kernel, dim3((unsigned)((n + SLS_BLOCK - 1) / SLS_BLOCK)), dim3(SLS_BLOCK), 0, (hipStream_t)stream, p, ncb, pt, pb,
                       pa, pw, v_G, v_A, v_B, v_w);
    return check_launch("gspl_spotless_mask_bwd (final)");
}

extern "C" int gspl_spotless_error_stats(int H, int W, int bins, const float* render, const float* gt, const float* thresholds, const float* edges,
                                         float* err, int32_t* counts, float* lower_mask, float* upper_mask, void* stream) {
    if (H < 1 || W < 1 || H > SLS_MAX_DIM || W > SLS_MAX_DIM) { set_error("gspl_spotless_error_stats", "H and W must be 1 .. 16384"); return GSPL_ERR_INVALID_ARG; }
    if (bins < 1 || bins > SLS_MAX_BINS) { set_error("gspl_spotless_error_stats", "bins must be 1 .. 15360"); return GSPL_ERR_INVALID_ARG; }
    if (!render || !gt || !thresholds || !edges || !err || !counts || !lower_mask || !upper_mask) return fail_arg("gspl_spotless_error_stats");
    const int tiles_x = (W + SLS_TILE - 1) / SLS_TILE, n_tiles = tiles_x * ((H + SLS_TILE - 1) / SLS_TILE);
    const int grid = n_tiles < 1024 ? n_tiles : 1024;
    hipLaunchKernelGGL(sls_error_stats_kernel, dim3(grid), dim3(SLS_BLOCK), (size_t)bins * sizeof(int32_t), (hipStream_t)stream, H, W, bins, tiles_x,
                       n_tiles, render, gt, thresholds, edges, err, counts, lower_mask, upper_mask);
    return check_launch("gspl_spotless_error_stats");
}

extern "C" int gspl_spotless_l1_partials(int64_t n) {
    if (n <= 0) return 1;
    return (int)((n + SLS_L1_PER_PARTIAL - 1) / SLS_L1_PER_PARTIAL);
}

extern "C" int gspl_spotless_masked_l1_fwd(int H, int W, const float* render, const float* gt, const float* mask, float* partials, float* out,
                                           void* stream) {
    if (H < 1 || W < 1 || H > SLS_MAX_DIM || W > SLS_MAX_DIM) { set_error("gspl_spotless_masked_l1_fwd", "H and W must be 1 .. 16384"); return GSPL_ERR_INVALID_ARG; }
    if (!render || !gt || !mask || !partials || !out) return fail_arg("gspl_spotless_masked_l1_fwd");
    const int64_t P = (int64_t)H * W;
    const int n = gspl_spotless_l1_partials(P);
    hipLaunchKernelGGL(sls_l1_partials_kernel, dim3(n), dim3(SLS_BLOCK), 0, (hipStream_t)stream, P, render, gt, mask, partials);
    if (const int rc = check_launch("gspl_spotless_masked_l1_fwd")) return rc;
    hipLaunchKernelGGL(sls_l1_final_kernel, dim3(1), dim3(SLS_BLOCK), 0, (hipStream_t)stream, n, (float)(3.0 * (double)P), partials, out);
    return check_launch("gspl_spotless_masked_l1_fwd");
}

extern "C" int gspl_spotless_masked_l1_bwd(int H, int W, const float* render, const float* gt, const float* mask, const float* grad_out,
                                           float* v_render, void* stream) {
    if (H < 1 || W < 1 || H > SLS_MAX_DIM || W > SLS_MAX_DIM) { set_error("gspl_spotless_masked_l1_bwd", "H and W must be 1 .. 16384"); return GSPL_ERR_INVALID_ARG; }
    if (!render || !gt || !mask || !grad_out || !v_render) return fail_arg("gspl_spotless_masked_l1_bwd");
    const int64_t P = (int64_t)H * W;
    hipLaunchKernelGGL(sls_l1_bwd_kernel, dim3((unsigned)((P + SLS_BLOCK - 1) / SLS_BLOCK)), dim3(SLS_BLOCK), 0, (hipStream_t)stream, P,
                       3.0 * (double)P, render, gt, mask, grad_out, v_render);
    return check_launch("gspl_spotless_masked_l1_bwd");
}

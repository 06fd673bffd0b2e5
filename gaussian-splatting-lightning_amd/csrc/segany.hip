// segany.hip — the SegAnyGS (SAGA) training step behind the renderer (gfx950): mask statistics, scale-aware pair labels and the
// correspondence loss with its backward.  The rules are those of include/gspl_hip.h section 24.
//
// What `SegAnySplatting.mask_preprocess` and `forward_with_loss_calculation` of the reference compute (internal/segany_splatting.py)
// after the choice of the sampled pixels, as a function of S pixels, N membership bits per pixel, S x C features and Ns x C gates:
//   stage 1  sga_cover_kernel reads the [N, H, W] byte masks once: per pixel the membership words (64 masks each), the cover count,
//            and per mask the area (a ballot's popcount per wave, integer atomics in LDS, then one per mask and workgroup).
//            sga_mean_kernel walks the words: the sum of the areas in 64-bit integers, rounded once, over cover + 1e-9.
//            sga_pack_kernel gathers the words of the sampled pixels in the order of descending scale.
//   stage 2  sga_head_kernel: head[n, s], the largest mask index <= scale_index[n] that holds pixel s.  sga_label_kernel: one lane per
//            pair, 16 x 64 pairs per workgroup, word-wise ANDs out of LDS; both triangles are written; the three counts are integers.
//   stage 3  sga_sample_kernel (the bilinear sample of the rendered map at the sampled pixels only), sga_norm_kernel (F.normalize per
//            scale), sga_range_kernel (the two constants of the pair weight), sga_pair_kernel (one lane per pair h <= j of a 16 x 16
//            tile: the Ns correlations as fmaf chains, the selection, the weighted sums; per-tile partial sums) and sga_final_kernel
//            (the partials added in tile order in float64).  No float atomics: two runs give the same bits.
//   backward sga_bwd_rows_kernel, one workgroup per pixel h: in chunks of 256 partners j it recomputes corr (the same chain, so the same
//            bits as the forward's), forms k_n(h, j) into LDS, then one lane per (n, c) adds k_n(h, j) X_n[j, c] over the chunk in
//            index order; the normalisation's adjoint, v_F and this pixel's share of v_gates follow.  sga_gates_kernel adds the shares
//            over s (one wave per value, lanes stride s, a fixed butterfly).  sga_scatter_kernel is the adjoint of the bilinear sample
//            with float atomics (samples share texels): the only sum here whose last bits depend on arrival order.
#include <cstdint>
#include "gspl_host.h"
#include "gspl_reduce.h"
#include "gspl_resample.h"

namespace gspl {
namespace {

constexpr int SGA_BLOCK = 256;
constexpr int SGA_MAX_S = 4096;        // every count is then <= 2^24: exact in float32
constexpr int SGA_MAX_MASKS = 1024;    // 16 words of 64 bits
constexpr int SGA_MAX_WORDS = SGA_MAX_MASKS / 64;
constexpr int SGA_MAX_SCALES = 16;     // a label is one bit of a uint16
constexpr int SGA_MAX_C = 64;
constexpr int SGA_MAX_DIM = 16384;
constexpr int SGA_TILE = 16;           // pairs per side of a loss tile
constexpr int SGA_LH = 16, SGA_LJ = 64;      // a label tile: 16 rows of 64 pairs

// ---- stage 1 -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SGA_BLOCK) void sga_cover_kernel(int N, int64_t P, const uint8_t* __restrict__ masks, int32_t* __restrict__ area,
                                                              int32_t* __restrict__ cover, uint64_t* __restrict__ packed) {
    __shared__ int32_t area_sh[SGA_MAX_MASKS];
    for (int k = threadIdx.x; k < N; k += SGA_BLOCK) area_sh[k] = 0;
    __syncthreads();
    const int NW = (N + 63) / 64, lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * SGA_BLOCK; base < P; base += (int64_t)gridDim.x * SGA_BLOCK) {      // (the same for every lane)
        const int64_t p = base + threadIdx.x;
        const bool valid = p < P;
        int cnt = 0;
        for (int w = 0; w < NW; ++w) {
            uint64_t word = 0;
            const int kn = min(64, N - 64 * w);
            for (int i = 0; i < kn; ++i) {
                const int k = 64 * w + i;
                const bool bit = valid && masks[(size_t)k * (size_t)P + (size_t)p] != 0;
                const uint64_t vote = __ballot(bit);
                if (lane == 0 && vote) atomicAdd(&area_sh[k], __popcll(vote));
                word |= (uint64_t)(bit ? 1 : 0) << i;
            }
            if (valid) packed[(size_t)w * (size_t)P + (size_t)p] = word;
            cnt += __popcll(word);
        }
        if (valid) cover[p] = cnt;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < N; k += SGA_BLOCK) {
        const int32_t n = area_sh[k];
        if (n) atomicAdd(&area[k], n);
    }
}

__global__ __launch_bounds__(SGA_BLOCK) void sga_mean_kernel(int N, int64_t P, const int32_t* __restrict__ area, const int32_t* __restrict__ cover,
                                                             const uint64_t* __restrict__ packed, float* __restrict__ mean_size) {
    __shared__ int32_t area_sh[SGA_MAX_MASKS];
    for (int k = threadIdx.x; k < N; k += SGA_BLOCK) area_sh[k] = area[k];
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * SGA_BLOCK + threadIdx.x;
    if (p >= P) return;
    const int NW = (N + 63) / 64;
    int64_t num = 0;
    for (int w = 0; w < NW; ++w) {
        uint64_t word = packed[(size_t)w * (size_t)P + (size_t)p];
        while (word) {
            num += area_sh[64 * w + (__ffsll((unsigned long long)word) - 1)];
            word &= word - 1;
        }
    }
    mean_size[p] = (float)num / ((float)cover[p] + 1e-9f);
}

// bits[s, w]: bit i = the mask order[64 w + i] holds pixel pixel_index[s]; an index outside the image or the masks sets nothing
__global__ __launch_bounds__(SGA_BLOCK) void sga_pack_kernel(int N, int64_t P, int S, const uint8_t* __restrict__ masks, const int32_t* __restrict__ order,
                                                             const int32_t* __restrict__ pixel_index, uint64_t* __restrict__ bits) {
    const int NW = (N + 63) / 64;
    const int t = blockIdx.x * SGA_BLOCK + threadIdx.x;
    if (t >= S * NW) return;
    const int s = t / NW, w = t % NW;
    const int64_t p = pixel_index[s];
    uint64_t word = 0;
    if (p >= 0 && p < P) {
        const int kn = min(64, N - 64 * w);
        for (int i = 0; i < kn; ++i) {
            const int m = order[64 * w + i];
            if (m >= 0 && m < N && masks[(size_t)m * (size_t)P + (size_t)p] != 0) word |= (uint64_t)1 << i;
        }
    }
    bits[t] = word;
}

// ---- stage 2 -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int sga_scale_index(const int32_t* __restrict__ scale_index, int n, int NW) { return min(max(scale_index[n], -1), 64 * NW - 1); }

__global__ __launch_bounds__(SGA_BLOCK) void sga_head_kernel(int S, int NW, int Ns, const uint64_t* __restrict__ bits, const int32_t* __restrict__ scale_index,
                                                             int32_t* __restrict__ head) {
    const int t = blockIdx.x * SGA_BLOCK + threadIdx.x;
    if (t >= Ns * S) return;
    const int n = t / S, s = t % S;
    const int si = sga_scale_index(scale_index, n, NW);
    int found = -1;
    for (int w = si >> 6; w >= 0 && found < 0; --w) {          // (si == -1: the shift gives -1, no word is read)
        uint64_t word = bits[(size_t)s * NW + w];
        if (w == (si >> 6) && (si & 63) != 63) word &= ((uint64_t)1 << ((si & 63) + 1)) - 1;
        if (word) found = 64 * w + 63 - __clzll((long long)word);
    }
    head[t] = found;
}

__global__ __launch_bounds__(SGA_BLOCK) void sga_label_kernel(int S, int NW, int Ns, const uint64_t* __restrict__ bits, const int32_t* __restrict__ scale_index,
                                                              const uint8_t* __restrict__ upper, const int32_t* __restrict__ head,
                                                              uint16_t* __restrict__ labels, int32_t* __restrict__ counts) {
    __shared__ uint64_t bj[SGA_MAX_WORDS][SGA_LJ], bh[SGA_MAX_WORDS][SGA_LH];
    __shared__ int32_t hj[SGA_MAX_SCALES][SGA_LJ], hh[SGA_MAX_SCALES][SGA_LH];
    __shared__ int32_t si_sh[SGA_MAX_SCALES], up_sh[SGA_MAX_SCALES], total[3];
    const int j0 = blockIdx.x * SGA_LJ, h0 = blockIdx.y * SGA_LH;
    for (int k = threadIdx.x; k < NW * SGA_LJ; k += SGA_BLOCK) {
        const int w = k / SGA_LJ, r = k % SGA_LJ;
        bj[w][r] = j0 + r < S ? bits[(size_t)(j0 + r) * NW + w] : 0;
    }
    for (int k = threadIdx.x; k < NW * SGA_LH; k += SGA_BLOCK) {
        const int w = k / SGA_LH, r = k % SGA_LH;
        bh[w][r] = h0 + r < S ? bits[(size_t)(h0 + r) * NW + w] : 0;
    }
    for (int k = threadIdx.x; k < Ns * SGA_LJ; k += SGA_BLOCK) {
        const int n = k / SGA_LJ, r = k % SGA_LJ;
        hj[n][r] = j0 + r < S ? head[(size_t)n * S + j0 + r] : -1;
    }
    for (int k = threadIdx.x; k < Ns * SGA_LH; k += SGA_BLOCK) {
        const int n = k / SGA_LH, r = k % SGA_LH;
        hh[n][r] = h0 + r < S ? head[(size_t)n * S + h0 + r] : -1;
    }
    if (threadIdx.x < Ns) {
        si_sh[threadIdx.x] = sga_scale_index(scale_index, threadIdx.x, NW);
        up_sh[threadIdx.x] = upper[threadIdx.x] != 0;
    }
    if (threadIdx.x < 3) total[threadIdx.x] = 0;
    __syncthreads();
    const int jl = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = j0 + jl;
    const uint16_t all = (uint16_t)((1u << Ns) - 1u);
    int n_neg = 0, n_pos = 0, n_inc = 0;
    for (int r = 0; r < SGA_LH / 4; ++r) {
        const int hl = wave * (SGA_LH / 4) + r, h = h0 + hl;
        if (h >= S || j >= S) continue;
        uint32_t lab = 0;
        for (int n = 0; n < Ns; ++n) {
            bool one = false;
            int w0 = 0;
            uint64_t first = ~(uint64_t)0;
            if (!up_sh[n]) {
                const int a = hh[n][hl];
                one = a >= 0 && a == hj[n][jl];
                const int lo = si_sh[n] + 1;                   // the masks of a smaller scale: indices >= lo
                w0 = lo >> 6;
                first = ~(uint64_t)0 << (lo & 63);
            }
            for (int w = w0; w < NW && !one; ++w) {
                const uint64_t common = bh[w][hl] & bj[w][jl] & (w == w0 ? first : ~(uint64_t)0);
                one = common != 0;
            }
            lab |= (one ? 1u : 0u) << n;
        }
        labels[(size_t)h * S + j] = (uint16_t)lab;
        n_neg += lab == 0;
        n_pos += lab == all;
        n_inc += lab != 0 && lab != all;
    }
    n_neg = wave_sum(n_neg), n_pos = wave_sum(n_pos), n_inc = wave_sum(n_inc);
    if (jl == 0) {
        atomicAdd(&total[0], n_neg);
        atomicAdd(&total[1], n_pos);
        atomicAdd(&total[2], n_inc);
    }
    __syncthreads();
    if (threadIdx.x < 3 && total[threadIdx.x]) atomicAdd(&counts[threadIdx.x], total[threadIdx.x]);
}

// ---- stage 3 -------------------------------------------------------------------------------------------------------------------------
struct SgaGrid {
    int Hr, Wr, mh, mw;       // the rendered map; the mask-sized grid the pixel indices address
    float sy, sx;             // (float)Hr / mh, (float)Wr / mw
};

__global__ __launch_bounds__(SGA_BLOCK) void sga_sample_kernel(int S, int C, SgaGrid g, const float* __restrict__ rendered, const int32_t* __restrict__ pixel_index,
                                                               float* __restrict__ F) {
    const int t = blockIdx.x * SGA_BLOCK + threadIdx.x;
    if (t >= S * C) return;
    const int s = t / C, c = t % C;
    const int p = pixel_index[s];
    float v = 0.f;
    if (p >= 0 && p < g.mh * g.mw) {
        const SlsAxis y = sls_axis(g.sy, p / g.mw, g.Hr), x = sls_axis(g.sx, p % g.mw, g.Wr);
        const float* plane = rendered + (size_t)c * g.Hr * g.Wr;
        const float t00 = plane[(size_t)y.i0 * g.Wr + x.i0], t01 = plane[(size_t)y.i0 * g.Wr + x.i1];
        const float t10 = plane[(size_t)y.i1 * g.Wr + x.i0], t11 = plane[(size_t)y.i1 * g.Wr + x.i1];
        const float top = fmaf(x.l, t01, x.h * t00), bot = fmaf(x.l, t11, x.h * t10);
        v = fmaf(y.l, bot, y.h * top);
    }
    F[t] = v;
}

__global__ __launch_bounds__(SGA_BLOCK) void sga_scatter_kernel(int S, int C, SgaGrid g, const float* __restrict__ v_F, const int32_t* __restrict__ pixel_index,
                                                                float* __restrict__ v_rendered) {
    const int t = blockIdx.x * SGA_BLOCK + threadIdx.x;
    if (t >= S * C) return;
    const int s = t / C, c = t % C;
    const int p = pixel_index[s];
    if (p < 0 || p >= g.mh * g.mw) return;
    const float v = v_F[t];
    if (v == 0.f) return;
    const SlsAxis y = sls_axis(g.sy, p / g.mw, g.Hr), x = sls_axis(g.sx, p % g.mw, g.Wr);
    float* plane = v_rendered + (size_t)c * g.Hr * g.Wr;
    const float top = y.h * v, bot = y.l * v;
    atomicAdd(plane + (size_t)y.i0 * g.Wr + x.i0, x.h * top);
    atomicAdd(plane + (size_t)y.i0 * g.Wr + x.i1, x.l * top);
    atomicAdd(plane + (size_t)y.i1 * g.Wr + x.i0, x.h * bot);
    atomicAdd(plane + (size_t)y.i1 * g.Wr + x.i1, x.l * bot);
}

// X[n, s, :] = (F[s] * gates[n]) / max(||F[s] * gates[n]||, 1e-12), norms[n, s] the norm itself
__global__ __launch_bounds__(SGA_BLOCK) void sga_norm_kernel(int S, int C, int Ns, const float* __restrict__ F, const float* __restrict__ gates,
                                                             float* __restrict__ X, float* __restrict__ norms) {
    const int t = blockIdx.x * SGA_BLOCK + threadIdx.x;
    if (t >= Ns * S) return;
    const int n = t / S, s = t % S;
    const float* f = F + (size_t)s * C;
    const float* g = gates + (size_t)n * C;
    float ss = 0.f;
    for (int c = 0; c < C; ++c) {
        const float u = f[c] * g[c];
        ss = fmaf(u, u, ss);
    }
    const float norm = sqrtf(ss), d = fmaxf(norm, 1e-12f);
    float* x = X + (size_t)t * C;
    for (int c = 0; c < C; ++c) x[c] = (f[c] * g[c]) / d;
    norms[t] = norm;
}

// params[0] = P = fl(a_max a_max), params[1] = R = max(P / fl(a_min a_min), 1)
__global__ __launch_bounds__(SGA_BLOCK) void sga_range_kernel(int S, const float* __restrict__ a, float* __restrict__ params) {
    __shared__ float lo_sh[SGA_BLOCK / 64], hi_sh[SGA_BLOCK / 64];
    float lo = a[0], hi = a[0];
    for (int s = threadIdx.x; s < S; s += SGA_BLOCK) {
        lo = fminf(lo, a[s]);
        hi = fmaxf(hi, a[s]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) lo_sh[threadIdx.x >> 6] = lo, hi_sh[threadIdx.x >> 6] = hi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SGA_BLOCK / 64; ++w) lo = fminf(lo, lo_sh[w]), hi = fmaxf(hi, hi_sh[w]);
        const float P = hi * hi;
        params[0] = P;
        params[1] = fmaxf(P / (lo * lo), 1.f);
    }
}

// the pair weight: every operation one float32 rounding, in the order of the reference's min-max normalised matrix
__device__ __forceinline__ float sga_weight(float P, float R, float ah, float aj) {
#pragma clang fp contract(off)
    const float prod = ah * aj;
    const float q = fmaxf(P / prod, 1.f);
    const float unit = (q - 1.f) / (R - 1.f);
    const float scaled = unit * 9.f;
    return scaled + 1.f;
}

struct SgaThresholds { float pos, neg; };
__device__ __forceinline__ SgaThresholds sga_thresholds(const int32_t* __restrict__ counts) {
    const float half = (float)counts[2] / 2.f;
    return SgaThresholds{half / (float)counts[1], half / (float)counts[0]};
}

// One 16 x 16 tile of pairs with tile row <= tile column; lane (ty, tx) owns the pair (h, j).  Partials per tile: pf [4] = the weighted
// sums over M+ and M-, the cosine sums of label 1 and label 0; pi [4] = |M+|, |M-|, the two cosine counts.
__global__ __launch_bounds__(SGA_BLOCK) void sga_pair_kernel(int S, int C, int Ns, const float* __restrict__ X, const uint16_t* __restrict__ labels,
                                                             const int32_t* __restrict__ counts, const float* __restrict__ a, const float* __restrict__ rnd,
                                                             const float* __restrict__ params, uint8_t* __restrict__ selected, float* __restrict__ weight,
                                                             float* __restrict__ pf, int32_t* __restrict__ pi) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;
    __shared__ float xh[SGA_TILE][SGA_MAX_C + 1], xj[SGA_TILE][SGA_MAX_C + 1];
    __shared__ float red_f[SGA_BLOCK / 64];
    __shared__ int red_i[SGA_BLOCK / 64];
    const int tx = threadIdx.x % SGA_TILE, ty = threadIdx.x / SGA_TILE;
    const int h = bi * SGA_TILE + ty, j = bj * SGA_TILE + tx;
    const bool active = h < S && j < S && h <= j, upper = active && h < j;
    const uint32_t lab = active ? labels[(size_t)h * S + j] : 0u;
    const uint32_t all = (1u << Ns) - 1u;
    float pos_sum = 0.f, neg_sum = 0.f, cos_pos = 0.f, cos_neg = 0.f;
    int n_cos_pos = 0, n_cos_neg = 0;
    bool hard_pos = false, hard_neg = false;
    const float twice = upper ? 2.f : 1.f;                     // the full matrix: both triangles and the diagonal
    for (int n = 0; n < Ns; ++n) {
        __syncthreads();                                       // (the last scale's rows are read)
        for (int k = threadIdx.x; k < SGA_TILE * C; k += SGA_BLOCK) {
            const int r = k / C, c = k % C;
            const int rh = bi * SGA_TILE + r, rj = bj * SGA_TILE + r;
            xh[r][c] = rh < S ? X[((size_t)n * S + rh) * C + c] : 0.f;
            xj[r][c] = rj < S ? X[((size_t)n * S + rj) * C + c] : 0.f;
        }
        __syncthreads();
        if (!active) continue;
        float corr = 0.f;
        for (int c = 0; c < C; ++c) corr = fmaf(xh[ty][c], xj[tx][c], corr);
        const bool one = (lab >> n) & 1u;
        if (one) {
            cos_pos = fmaf(twice, corr, cos_pos);
            n_cos_pos += upper ? 2 : 1;
            pos_sum += corr;
            hard_pos |= corr < 0.75f;
        } else {
            cos_neg = fmaf(twice, corr, cos_neg);
            n_cos_neg += upper ? 2 : 1;
            neg_sum += fmaxf(corr, 0.f);
            hard_neg |= corr > 0.5f;
        }
    }
    float loss_pos = 0.f, loss_neg = 0.f;
    int n_pos = 0, n_neg = 0;
    if (active) {
        const float w = sga_weight(params[0], params[1], a[h], a[j]);
        if (weight) weight[(size_t)h * S + j] = weight[(size_t)j * S + h] = w;
        if (upper) {
            const SgaThresholds t = sga_thresholds(counts);
            const float r = rnd[(size_t)h * S + j];
            const bool inconsistent = lab != 0u && lab != all;
            const bool in_pos = (lab == all && r < t.pos) || hard_pos || inconsistent;
            const bool in_neg = (lab == 0u && r < t.neg) || hard_neg || inconsistent;
            selected[(size_t)h * S + j] = (uint8_t)((in_pos ? 1 : 0) | (in_neg ? 2 : 0));
            if (in_pos) loss_pos = w * pos_sum, n_pos = 1;
            if (in_neg) loss_neg = w * neg_sum, n_neg = 1;
        }
    }
    const float f0 = block_sum<SGA_BLOCK>(loss_pos, red_f), f1 = block_sum<SGA_BLOCK>(loss_neg, red_f);
    const float f2 = block_sum<SGA_BLOCK>(cos_pos, red_f), f3 = block_sum<SGA_BLOCK>(cos_neg, red_f);
    const int i0 = block_sum<SGA_BLOCK>(n_pos, red_i), i1 = block_sum<SGA_BLOCK>(n_neg, red_i);
    const int i2 = block_sum<SGA_BLOCK>(n_cos_pos, red_i), i3 = block_sum<SGA_BLOCK>(n_cos_neg, red_i);
    if (threadIdx.x == 0) {
        const size_t at = ((size_t)bi * gridDim.x + bj) * 4;
        pf[at] = f0, pf[at + 1] = f1, pf[at + 2] = f2, pf[at + 3] = f3;
        pi[at] = i0, pi[at + 1] = i1, pi[at + 2] = i2, pi[at + 3] = i3;
    }
}

// the tiles' partials in tile order, in float64: out [3] = loss, cosine_pos, cosine_neg; sel_counts [2] = |M+|, |M-|
__global__ __launch_bounds__(SGA_BLOCK) void sga_final_kernel(int nt, int Ns, const float* __restrict__ pf, const int32_t* __restrict__ pi,
                                                              float* __restrict__ out, int32_t* __restrict__ sel_counts) {
    __shared__ double sh[8][SGA_BLOCK / 64];
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int t = threadIdx.x; t < nt * nt; t += SGA_BLOCK) {
        if (t / nt > t % nt) continue;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            acc[k] += (double)pf[(size_t)t * 4 + k];
            acc[4 + k] += (double)pi[(size_t)t * 4 + k];      // (counts: integers below 2^53, exact)
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double v = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double v[8];
        for (int k = 0; k < 8; ++k) v[k] = ((sh[k][0] + sh[k][1]) + sh[k][2]) + sh[k][3];
        out[0] = (float)(-v[0] / ((double)Ns * v[4]) + v[1] / ((double)Ns * v[5]));
        out[1] = (float)(v[2] / v[6]);
        out[2] = (float)(v[3] / v[7]);
        sel_counts[0] = (int32_t)v[4];
        sel_counts[1] = (int32_t)v[5];
    }
}

// One workgroup per pixel h.  dG [S, Ns, C]: this pixel's share of v_gates.
__global__ __launch_bounds__(SGA_BLOCK) void sga_bwd_rows_kernel(int S, int C, int Ns, const float* __restrict__ X, const float* __restrict__ norms,
                                                                 const float* __restrict__ F, const float* __restrict__ gates,
                                                                 const uint16_t* __restrict__ labels, const float* __restrict__ a,
                                                                 const float* __restrict__ params, const uint8_t* __restrict__ selected,
                                                                 const int32_t* __restrict__ sel_counts, const float* __restrict__ grad_out,
                                                                 float* __restrict__ v_F, float* __restrict__ dG) {
    __shared__ float xh[SGA_MAX_SCALES * SGA_MAX_C], dx[SGA_MAX_SCALES * SGA_MAX_C], k_sh[SGA_MAX_SCALES][SGA_BLOCK], dot_sh[SGA_MAX_SCALES];
    constexpr int PER = SGA_MAX_SCALES * SGA_MAX_C / SGA_BLOCK;      // (n, c) values per lane
    const int h = blockIdx.x, tid = threadIdx.x, NC = Ns * C;
    for (int o = tid; o < NC; o += SGA_BLOCK) xh[o] = X[((size_t)(o / C) * S + h) * C + o % C];
    const float g = grad_out[0];
    const float inv_pos = g / ((float)Ns * (float)sel_counts[0]), inv_neg = g / ((float)Ns * (float)sel_counts[1]);
    const float P = params[0], R = params[1], ah = a[h];
    float acc[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) acc[q] = 0.f;
    __syncthreads();
    for (int j0 = 0; j0 < S; j0 += SGA_BLOCK) {
        const int j = j0 + tid;
        uint32_t sel = 0;
        if (j < S && j != h) sel = selected[(size_t)min(h, j) * S + max(h, j)];
        if (sel) {
            const uint32_t lab = labels[(size_t)h * S + j];
            const float w = sga_weight(P, R, ah, a[j]);
            const float k_pos = -(w * inv_pos), k_neg = w * inv_neg;
            for (int n = 0; n < Ns; ++n) {
                const float* xj = X + ((size_t)n * S + j) * C;
                const float* xa = h < j ? xh + n * C : xj;      // the forward's chain has the smaller index on the left: the same bits
                const float* xb = h < j ? xj : xh + n * C;
                float corr = 0.f;
                for (int c = 0; c < C; ++c) corr = fmaf(xa[c], xb[c], corr);
                const bool one = (lab >> n) & 1u;
                float k = 0.f;
                if ((sel & 1u) && one) k = k_pos;
                if ((sel & 2u) && !one && corr > 0.f) k = k_neg;
                k_sh[n][tid] = k;
            }
        } else {
            for (int n = 0; n < Ns; ++n) k_sh[n][tid] = 0.f;
        }
        __syncthreads();
        const int count = min(SGA_BLOCK, S - j0);
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int o = tid + q * SGA_BLOCK;
            if (o < NC) {
                const int n = o / C, c = o % C;
                const float* col = X + ((size_t)n * S + j0) * C + c;
                float sum = acc[q];
                for (int jj = 0; jj < count; ++jj) sum = fmaf(k_sh[n][jj], col[(size_t)jj * C], sum);
                acc[q] = sum;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int o = tid + q * SGA_BLOCK;
        if (o < NC) dx[o] = acc[q];
    }
    __syncthreads();
    if (tid < Ns) {
        float dot = 0.f;
        for (int c = 0; c < C; ++c) dot = fmaf(xh[tid * C + c], dx[tid * C + c], dot);
        dot_sh[tid] = dot;
    }
    __syncthreads();
    float du[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int o = tid + q * SGA_BLOCK;
        du[q] = 0.f;
        if (o < NC) {
            const int n = o / C;
            const float norm = norms[(size_t)n * S + h];
            // F.normalize: x / max(norm, 1e-12); below the clamp the denominator is a constant
            du[q] = norm >= 1e-12f ? (dx[o] - xh[o] * dot_sh[n]) / norm : dx[o] / 1e-12f;
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int o = tid + q * SGA_BLOCK;
        if (o < NC) {
            dx[o] = du[q];
            dG[(size_t)h * NC + o] = du[q] * F[(size_t)h * C + o % C];
        }
    }
    __syncthreads();
    if (tid < C) {
        float sum = 0.f;
        for (int n = 0; n < Ns; ++n) sum = fmaf(dx[n * C + tid], gates[n * C + tid], sum);
        v_F[(size_t)h * C + tid] = sum;
    }
}

// one wave per value of v_gates: lanes stride s, then a fixed butterfly
__global__ __launch_bounds__(64) void sga_gates_kernel(int S, int NC, const float* __restrict__ dG, float* __restrict__ v_gates) {
    const int o = blockIdx.x, lane = threadIdx.x;
    float acc = 0.f;
    for (int s = lane; s < S; s += 64) acc += dG[(size_t)s * NC + o];
    acc = wave_sum(acc);
    if (lane == 0) v_gates[o] = acc;
}

bool sga_dim(int n) { return n >= 1 && n <= SGA_MAX_DIM; }

int sga_masks(const char* who, int N, int H, int W) {
    if (N < 1 || N > SGA_MAX_MASKS) { set_error(who, "N (masks) must be 1 .. 1024"); return GSPL_ERR_INVALID_ARG; }
    if (!sga_dim(H) || !sga_dim(W)) { set_error(who, "H and W must be 1 .. 16384"); return GSPL_ERR_INVALID_ARG; }
    return GSPL_OK;
}

int sga_pairs(const char* who, int S, int Ns) {
    if (S < 1 || S > SGA_MAX_S) { set_error(who, "S (sampled pixels) must be 1 .. 4096"); return GSPL_ERR_INVALID_ARG; }
    if (Ns < 1 || Ns > SGA_MAX_SCALES) { set_error(who, "Ns (scales) must be 1 .. 16"); return GSPL_ERR_INVALID_ARG; }
    return GSPL_OK;
}

int sga_loss_shape(const char* who, int S, int C, int Ns, int Hr, int Wr, int mh, int mw, SgaGrid& g) {
    if (const int rc = sga_pairs(who, S, Ns)) return rc;
    if (C < 4 || C > SGA_MAX_C || C % 4) { set_error(who, "C must be a multiple of 4, 4 .. 64"); return GSPL_ERR_INVALID_ARG; }
    if (!sga_dim(Hr) || !sga_dim(Wr) || !sga_dim(mh) || !sga_dim(mw)) { set_error(who, "every image dimension must be 1 .. 16384"); return GSPL_ERR_INVALID_ARG; }
    g = SgaGrid{Hr, Wr, mh, mw, (float)Hr / (float)mh, (float)Wr / (float)mw};
    return GSPL_OK;
}

int sga_tiles(int S) { return (S + SGA_TILE - 1) / SGA_TILE; }

struct SgaWork { size_t X, norms, params, pf, pi, dG, total; };
SgaWork sga_work(int S, int C, int Ns) {
    const size_t nt = (size_t)sga_tiles(S);
    Carve c;
    SgaWork w;
    w.X = c.take((size_t)Ns * S * C * sizeof(float));
    w.norms = c.take((size_t)Ns * S * sizeof(float));
    w.params = c.take(2 * sizeof(float));
    w.pf = c.take(nt * nt * 4 * sizeof(float));
    w.pi = c.take(nt * nt * 4 * sizeof(int32_t));
    w.dG = c.take((size_t)S * Ns * C * sizeof(float));
    w.total = c.off;
    return w;
}

unsigned sga_grid(int64_t n) { return (unsigned)((n + SGA_BLOCK - 1) / SGA_BLOCK); }

}  // namespace
}  // namespace gspl

using namespace gspl;

extern "C" int gspl_segany_mask_stats(int N, int H, int W, const uint8_t* masks, int32_t* area, int32_t* cover, float* mean_size,
                                      uint64_t* packed, void* stream) {
    if (const int rc = sga_masks("gspl_segany_mask_stats", N, H, W)) return rc;
    if (!masks || !area || !cover || !mean_size || !packed) return fail_arg("gspl_segany_mask_stats");
    const int64_t P = (int64_t)H * W;
    const int64_t blocks = (P + SGA_BLOCK - 1) / SGA_BLOCK;
    hipLaunchKernelGGL(sga_cover_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(SGA_BLOCK), 0, (hipStream_t)stream, N, P, masks, area,
                       cover, packed);
    if (const int rc = check_launch("gspl_segany_mask_stats (cover)")) return rc;
    hipLaunchKernelGGL(sga_mean_kernel, dim3((unsigned)blocks), dim3(SGA_BLOCK), 0, (hipStream_t)stream, N, P, area, cover, packed, mean_size);
    return check_launch("gspl_segany_mask_stats (mean)");
}

extern "C" int gspl_segany_pack_membership(int N, int H, int W, int S, const uint8_t* masks, const int32_t* order, const int32_t* pixel_index,
                                           uint64_t* bits, void* stream) {
    if (const int rc = sga_masks("gspl_segany_pack_membership", N, H, W)) return rc;
    if (S < 1 || S > SGA_MAX_S) { set_error("gspl_segany_pack_membership", "S (sampled pixels) must be 1 .. 4096"); return GSPL_ERR_INVALID_ARG; }
    if (!masks || !order || !pixel_index || !bits) return fail_arg("gspl_segany_pack_membership");
    const int NW = (N + 63) / 64;
    hipLaunchKernelGGL(sga_pack_kernel, dim3(sga_grid((int64_t)S * NW)), dim3(SGA_BLOCK), 0, (hipStream_t)stream, N, (int64_t)H * W, S, masks, order,
                       pixel_index, bits);
    return check_launch("gspl_segany_pack_membership");
}

extern "C" int gspl_segany_pair_labels(int S, int N, int Ns, const uint64_t* bits, const int32_t* scale_index, const uint8_t* upper, int32_t* head,
                                       uint16_t* labels, int32_t* counts, void* stream) {
    if (const int rc = sga_pairs("gspl_segany_pair_labels", S, Ns)) return rc;
    if (N < 1 || N > SGA_MAX_MASKS) { set_error("gspl_segany_pair_labels", "N (masks) must be 1 .. 1024"); return GSPL_ERR_INVALID_ARG; }
    if (!bits || !scale_index || !upper || !head || !labels || !counts) return fail_arg("gspl_segany_pair_labels");
    const int NW = (N + 63) / 64;
    hipLaunchKernelGGL(sga_head_kernel, dim3(sga_grid((int64_t)Ns * S)), dim3(SGA_BLOCK), 0, (hipStream_t)stream, S, NW, Ns, bits, scale_index, head);
    if (const int rc = check_launch("gspl_segany_pair_labels (head)")) return rc;
    const dim3 grid((S + SGA_LJ - 1) / SGA_LJ, (S + SGA_LH - 1) / SGA_LH);
    hipLaunchKernelGGL(sga_label_kernel, grid, dim3(SGA_BLOCK), 0, (hipStream_t)stream, S, NW, Ns, bits, scale_index, upper, head, labels, counts);
    return check_launch("gspl_segany_pair_labels");
}

extern "C" size_t gspl_segany_loss_workspace_bytes(int S, int C, int Ns) {
    if (S < 1 || S > SGA_MAX_S || Ns < 1 || Ns > SGA_MAX_SCALES || C < 4 || C > SGA_MAX_C) return 0;
    return sga_work(S, C, Ns).total;
}

extern "C" int gspl_segany_loss_fwd(int S, int C, int Ns, int Hr, int Wr, int mh, int mw, const float* rendered, const int32_t* pixel_index,
                                    const float* gates, const uint16_t* labels, const int32_t* counts, const float* a, const float* rnd,
                                    float* F, float* out, int32_t* sel_counts, uint8_t* selected, float* weight, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    const char* who = "gspl_segany_loss_fwd";
    SgaGrid g;
    if (const int rc = sga_loss_shape(who, S, C, Ns, Hr, Wr, mh, mw, g)) return rc;
    if (!rendered || !pixel_index || !gates || !labels || !counts || !a || !rnd || !F || !out || !sel_counts || !selected || !workspace) return fail_arg(who);
    const SgaWork w = sga_work(S, C, Ns);
    if (workspace_bytes < w.total) return fail_ws(who);
    char* ws = (char*)workspace;
    float *X = (float*)(ws + w.X), *norms = (float*)(ws + w.norms), *params = (float*)(ws + w.params), *pf = (float*)(ws + w.pf);
    int32_t* pi = (int32_t*)(ws + w.pi);
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sga_sample_kernel, dim3(sga_grid((int64_t)S * C)), dim3(SGA_BLOCK), 0, s, S, C, g, rendered, pixel_index, F);
    if (const int rc = check_launch("gspl_segany_loss_fwd (sample)")) return rc;
    hipLaunchKernelGGL(sga_norm_kernel, dim3(sga_grid((int64_t)Ns * S)), dim3(SGA_BLOCK), 0, s, S, C, Ns, F, gates, X, norms);
    if (const int rc = check_launch("gspl_segany_loss_fwd (normalise)")) return rc;
    hipLaunchKernelGGL(sga_range_kernel, dim3(1), dim3(SGA_BLOCK), 0, s, S, a, params);
    if (const int rc = check_launch("gspl_segany_loss_fwd (range)")) return rc;
    const int nt = sga_tiles(S);
    hipLaunchKernelGGL(sga_pair_kernel, dim3(nt, nt), dim3(SGA_BLOCK), 0, s, S, C, Ns, X, labels, counts, a, rnd, params, selected, weight, pf, pi);
    if (const int rc = check_launch("gspl_segany_loss_fwd (pairs)")) return rc;
    hipLaunchKernelGGL(sga_final_kernel, dim3(1), dim3(SGA_BLOCK), 0, s, nt, Ns, pf, pi, out, sel_counts);
    return check_launch("gspl_segany_loss_fwd (final)");
}

extern "C" int gspl_segany_loss_bwd(int S, int C, int Ns, int Hr, int Wr, int mh, int mw, const int32_t* pixel_index, const float* gates,
                                    const uint16_t* labels, const float* a, const uint8_t* selected, const int32_t* sel_counts, const float* F,
                                    const float* grad_out, float* v_F, float* v_gates, float* v_rendered, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    const char* who = "gspl_segany_loss_bwd";
    SgaGrid g;
    if (const int rc = sga_loss_shape(who, S, C, Ns, Hr, Wr, mh, mw, g)) return rc;
    if (!pixel_index || !gates || !labels || !a || !selected || !sel_counts || !F || !grad_out || !v_F || !v_gates || !workspace) return fail_arg(who);
    const SgaWork w = sga_work(S, C, Ns);
    if (workspace_bytes < w.total) return fail_ws(who);
    char* ws = (char*)workspace;
    float *X = (float*)(ws + w.X), *norms = (float*)(ws + w.norms), *params = (float*)(ws + w.params), *dG = (float*)(ws + w.dG);
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sga_norm_kernel, dim3(sga_grid((int64_t)Ns * S)), dim3(SGA_BLOCK), 0, s, S, C, Ns, F, gates, X, norms);
    if (const int rc = check_launch("gspl_segany_loss_bwd (normalise)")) return rc;
    hipLaunchKernelGGL(sga_range_kernel, dim3(1), dim3(SGA_BLOCK), 0, s, S, a, params);
    if (const int rc = check_launch("gspl_segany_loss_bwd (range)")) return rc;
    hipLaunchKernelGGL(sga_bwd_rows_kernel, dim3(S), dim3(SGA_BLOCK), 0, s, S, C, Ns, X, norms, F, gates, labels, a, params, selected, sel_counts,
                       grad_out, v_F, dG);
    if (const int rc = check_launch("gspl_segany_loss_bwd (rows)")) return rc;
    hipLaunchKernelGGL(sga_gates_kernel, dim3(Ns * C), dim3(64), 0, s, S, Ns * C, dG, v_gates);
    if (const int rc = check_launch("gspl_segany_loss_bwd (gates)")) return rc;
    if (v_rendered) {
        hipLaunchKernelGGL(sga_scatter_kernel, dim3(sga_grid((int64_t)S * C)), dim3(SGA_BLOCK), 0, s, S, C, g, v_F, pixel_index, v_rendered);
        return check_launch("gspl_segany_loss_bwd (scatter)");
    }
    return GSPL_OK;
}

// appearance.hip — the per-Gaussian appearance MLP of the appearance-embedding route, fused, forward and backward (gfx950).
//
// What `Model.forward` of internal/renderers/gsplat_appearance_embedding_renderer.py computes with `tcnn: false`, for ONE
// appearance id per call (include/gspl_hip.h section 21): [features | embedding | encoded view direction] -> Linear/ReLU ... ->
// Linear -> Sigmoid.  Exact fp32 on the f32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, no reduced precision).
//
// Orientation: the ROW (Gaussian) is on the lane (j = lane & 31), the NEURON in the 16 accumulator registers: register r of lane
// half h = lane >> 5 is neuron 8 (r >> 2) + 4 h + (r & 3) of its 32-block.  A layer's accumulator is then the next layer's B operand
// as it stands (k step r: half h supplies that neuron), and the weights are the A operand, read from one LDS image per layer
// [32 IB rows][32 KB + 1] (odd stride: both the row-on-lane read of the forward and the column-on-lane read of W^T in the backward
// are free of bank conflicts).  The embedding is folded into the first bias once per workgroup, so layer 1 has K = F (+ encoding).
//
// A workgroup (256 threads, 4 waves) walks row blocks of 256 rows, block b of workgroup g being g + b * gridDim.x (static).  The
// visible rows of a block are compacted into an index list in LDS; a wave takes tiles of 32 compacted rows, so a masked row costs
// no arithmetic (a tile is skipped or shorter).  Masked rows get zeros from the thread that owns them.
//
// Backward: the hidden activations are RECOMPUTED (nothing but the output was saved).  Weight gradients sum over the lane index:
// delta and the layer's input go through LDS once per layer (delta transposed to [neuron][row], the input as [row][k]).  That
// product is the WORKGROUP's work: after a barrier, 32x32 tile o of the layer's gradient belongs to wave o % 4, which sums it over
// the tiles the waves ran this round, in wave order, and keeps it in registers for the whole launch (a wave that kept every tile
// of every layer for its own rows would need more than the register file).  At the end each wave writes the tiles it owns: ONE
// partial per workgroup; ap_reduce_kernel sums the partials in workgroup order, and derives v_embedding and v_W0[:, F:F+E] from
// the reduced first-layer bias gradient.  No float atomics anywhere: the same bits every run.
#include <cstdint>
#include "gspl_host.h"

namespace gspl {

using f32x16 = __attribute__((ext_vector_type(16))) float;

static constexpr int AP_TILE = 32;          // rows of a wave tile (the MFMA's N)
static constexpr int AP_BLOCK = 256;        // rows of a workgroup pass = threads of a workgroup
static constexpr int AP_GRID = 256;         // workgroups at most (one per CU: a wave per SIMD, the accumulators fill the register file)
static constexpr int AP_MAX_LAYERS = 4;
static constexpr int AP_MAX_E = 256;
static constexpr int AP_MAX_KB1 = 6;
static constexpr int AP_LDS_BYTES = 160 * 1024;
enum { AP_NORMALIZE = 1, AP_SIGMOID = 2 };

struct ApNet {
    int N, F, E, P, K1, H, n_out, n_freq, flags, n_blocks, n_waves;
    const float* features; const uint8_t* mask; const float* means; const float* cam; const float* emb;
    const float* W[AP_MAX_LAYERS]; const float* B[AP_MAX_LAYERS];
};

// LDS map, in floats.  KB1: 32-blocks of the first layer's K, HB: of the hidden width, NL: linear layers.
template <int KB1, int HB, int NL>
struct ApGeom {
    static constexpr int rb(int l) { return l == NL - 1 ? 1 : HB; }
    static constexpr int cb(int l) { return l == 0 ? KB1 : HB; }
    static constexpr int stride(int l) { return 32 * cb(l) + 1; }
    static constexpr int w_off(int l) { int o = 0; for (int i = 0; i < l; ++i) o += 32 * rb(i) * stride(i); return o; }
    static constexpr int bias_off = w_off(NL);
    static constexpr int ehat_off = bias_off + 64 * NL;
    static constexpr int idx_off = ehat_off + AP_MAX_E;
    static constexpr int vis_off = idx_off + AP_BLOCK;
    static constexpr int cnt_off = vis_off + AP_BLOCK;
    static constexpr int wave_off = cnt_off + 8;
    static constexpr int xs = 32 * KB1 + 1, as = 32 * HB + 1, ds = 33;
    static constexpr int per_wave(bool bwd) { return 32 * xs + (bwd ? 32 * as + 32 * HB * ds : 0); }
    static constexpr int total(bool bwd, int n_waves) { return wave_off + n_waves * per_wave(bwd); }
};

__host__ __device__ inline int ap_rows(const ApNet& a, int l, int NL) { return l == NL - 1 ? a.n_out : a.H; }
__host__ __device__ inline int ap_cols(const ApNet& a, int l) { return l == 0 ? a.K1 : a.H; }          // without the embedding columns
__host__ __device__ inline int ap_in(const ApNet& a, int l) { return l == 0 ? a.K1 + a.E : a.H; }     // torch.nn.Linear's in_features
__host__ __device__ inline int ap_compact_total(const ApNet& a, int NL) {
    int o = 0;
    for (int l = 0; l < NL; ++l) o += ap_rows(a, l, NL) * (ap_cols(a, l) + 1);
    return o;
}

__device__ __forceinline__ int ap_perm(int r, int h) { return 8 * (r >> 2) + 4 * h + (r & 3); }
__device__ __forceinline__ void ap_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
#define AP_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// out = bias + W x, x [row][k] in LDS (the first layer)
template <int IB, int KB>
__device__ __forceinline__ void ap_dense_lds(const float* Wimg, int S, const float* bias, const float* Xs, int XS, f32x16 (&out)[IB], int j, int h) {
#pragma unroll
    for (int ib = 0; ib < IB; ++ib)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[ib][r] = bias[32 * ib + ap_perm(r, h)];
#pragma unroll 8
    for (int s = 0; s < 16 * KB; ++s) {
        const float b = Xs[j * XS + 2 * s + h];
#pragma unroll
        for (int ib = 0; ib < IB; ++ib) out[ib] = AP_MFMA(Wimg[(32 * ib + j) * S + 2 * s + h], b, out[ib]);
    }
}

// out = bias + W x, x the accumulator tiles of the layer before
template <int IB, int KB>
__device__ __forceinline__ void ap_dense(const float* Wimg, int S, const float* bias, const f32x16 (&in)[KB], f32x16 (&out)[IB], int j, int h) {
#pragma unroll
    for (int ib = 0; ib < IB; ++ib) {
#pragma unroll
        for (int r = 0; r < 16; ++r) out[ib][r] = bias[32 * ib + ap_perm(r, h)];
        const float* w = Wimg + (32 * ib + j) * S + 4 * h;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) out[ib] = AP_MFMA(w[32 * kb + 8 * (r >> 2) + (r & 3)], in[kb][r], out[ib]);
    }
}

// out[kb] = W^T d for kb < kb_count (d: IB tiles; only registers r < RMAX of d can be non-zero)
template <int IB, int KB, int RMAX>
__device__ __forceinline__ void ap_dense_t(const float* Wimg, int S, const f32x16 (&d)[IB], f32x16 (&out)[KB], int kb_count, int j, int h) {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) out[kb][r] = 0.f;
        if (kb < kb_count) {
#pragma unroll
            for (int ib = 0; ib < IB; ++ib)
#pragma unroll
                for (int r = 0; r < RMAX; ++r) out[kb] = AP_MFMA(Wimg[(32 * ib + ap_perm(r, h)) * S + 32 * kb + j], d[ib][r], out[kb]);
        }
    }
}

// delta tiles -> Ds [neuron][row] (stride 33)
template <int IB>
__device__ __forceinline__ void ap_put_delta(float* Ds, const f32x16 (&d)[IB], int j, int h) {
#pragma unroll
    for (int ib = 0; ib < IB; ++ib)
#pragma unroll
        for (int r = 0; r < 16; ++r) Ds[(32 * ib + ap_perm(r, h)) * 33 + j] = d[ib][r];
}
// activation tiles -> As [row][k]
template <int KB>
__device__ __forceinline__ void ap_put_act(float* As, int AS, const f32x16 (&x)[KB], int j, int h) {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) As[j * AS + 32 * kb + ap_perm(r, h)] = x[kb][r];
}
// The weight gradient of one layer, by the whole workgroup: the waves that ran a tile this round have left delta [neuron][row] (Ds) and
// the layer's input [row][k] (As, or Xs for the first layer) in their LDS regions.  Output tile o = ib * KB + kb belongs to wave o % 4,
// which sums it over the active regions in wave order; wave 0 also sums the bias gradient of neuron `lane`.
template <int IB, int KB>
__device__ __forceinline__ void ap_wgrad(const float* regions, int per_wave, int ds_off, int in_off, int IS, int n_active,
                                         f32x16 (&acc)[(IB * KB + 3) / 4], float& gb, int wave, int lane) {
    const int j = lane & 31, h = lane >> 5;
#pragma unroll
    for (int q = 0; q < (IB * KB + 3) / 4; ++q) {
        const int o = wave + 4 * q;
        if (o < IB * KB) {
            const int ib = o / KB, kb = o - ib * KB;
            for (int w = 0; w < n_active; ++w) {
                const float* Ds = regions + w * per_wave + ds_off + (32 * ib + j) * 33 + h;
                const float* In = regions + w * per_wave + in_off + h * IS + 32 * kb + j;
#pragma unroll
                for (int s = 0; s < 16; ++s) acc[q] = AP_MFMA(Ds[2 * s], In[2 * s * IS], acc[q]);
            }
        }
    }
    if (wave == 0 && lane < 32 * IB) {
        for (int w = 0; w < n_active; ++w) {
            const float* Ds = regions + w * per_wave + ds_off + lane * 33;
            float sum = 0.f;
#pragma unroll 8
            for (int row = 0; row < 32; ++row) sum += Ds[row];
            gb += sum;
        }
    }
}

// the tiles of a [rows, cols] gradient this wave owns -> the workgroup's partial (compact, row-major)
template <int IB, int KB>
__device__ __forceinline__ void ap_dump(float* dst, int rows, int cols, const f32x16 (&acc)[(IB * KB + 3) / 4], int wave, int lane) {
    const int j = lane & 31, h = lane >> 5;
#pragma unroll
    for (int q = 0; q < (IB * KB + 3) / 4; ++q) {
        const int o = wave + 4 * q;
        if (o < IB * KB) {
            const int ib = o / KB, kb = o - ib * KB;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = 32 * ib + ap_perm(r, h), k = 32 * kb + j;
                if (i < rows && k < cols) dst[i * cols + k] = acc[q][r];
            }
        }
    }
}

template <int KB>
__device__ __forceinline__ void ap_relu(f32x16 (&x)[KB]) {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) x[kb][r] = fmaxf(x[kb][r], 0.f);
}
template <int KB>
__device__ __forceinline__ void ap_relu_bwd(f32x16 (&d)[KB], const f32x16 (&act)[KB]) {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) d[kb][r] = act[kb][r] > 0.f ? d[kb][r] : 0.f;
}

// entry p of the encoded direction: x, sin(2^0 x), cos(2^0 x), sin(2^1 x), ...
__device__ __forceinline__ float ap_encode(const float (&d)[3], int p) {
    if (p < 3) return d[p];
    const int t = p - 3, f = t / 6, w = t % 6;
    const float x = ldexpf(d[w % 3], f);
    return w < 3 ? sinf(x) : cosf(x);
}

template <int KB1, int HB, int NL, bool BWD>
__global__ __launch_bounds__(AP_BLOCK) void ap_kernel(ApNet a, float* __restrict__ out, const float* __restrict__ v_out,
                                                      float* __restrict__ v_features, float* __restrict__ partials) {
    using G = ApGeom<KB1, HB, NL>;
    extern __shared__ __attribute__((aligned(16))) float ap_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    float* bias = ap_lds + G::bias_off;
    float* ehat = ap_lds + G::ehat_off;
    int* idx = reinterpret_cast<int*>(ap_lds + G::idx_off);
    int* visf = reinterpret_cast<int*>(ap_lds + G::vis_off);
    int* wcnt = reinterpret_cast<int*>(ap_lds + G::cnt_off);
    const bool normalize = a.flags & AP_NORMALIZE, sigmoid = a.flags & AP_SIGMOID;
    const bool want_w = BWD && partials != nullptr, want_f = BWD && v_features != nullptr;

    // ---- once per workgroup: weight images, the (normalised) embedding, the biases with the embedding folded into the first
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int S = G::stride(l), R = 32 * G::rb(l), rows = ap_rows(a, l, NL), cols = ap_cols(a, l), in = ap_in(a, l);
        float* img = ap_lds + G::w_off(l);
        for (int e = tid; e < R * S; e += AP_BLOCK) {
            const int i = e / S, k = e - i * S;
            float v = 0.f;
            if (i < rows && k < cols) v = a.W[l][(size_t)i * in + ((l == 0 && k >= a.F) ? k + a.E : k)];
            img[e] = v;
        }
    }
    for (int e = tid; e < a.E; e += AP_BLOCK) ehat[e] = a.emb[e];
    __syncthreads();
    if (normalize && a.E > 0) {
        float ss = 0.f;
        for (int e = 0; e < a.E; ++e) ss = fmaf(ehat[e], ehat[e], ss);
        const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
        __syncthreads();
        for (int e = tid; e < a.E; e += AP_BLOCK) ehat[e] *= inv;
        __syncthreads();
    }
    for (int e = tid; e < 64 * NL; e += AP_BLOCK) {
        const int l = e >> 6, i = e & 63;
        float v = 0.f;
        if (i < ap_rows(a, l, NL)) {
            v = a.B[l][i];
            if (l == 0) {
                const float* w = a.W[0] + (size_t)i * ap_in(a, 0) + a.F;
                for (int c = 0; c < a.E; ++c) v = fmaf(w[c], ehat[c], v);
            }
        }
        bias[e] = v;
    }
    __syncthreads();

    float* regions = ap_lds + G::wave_off;
    constexpr int per_wave = G::per_wave(BWD), as_off = 32 * G::xs, ds_off = 32 * G::xs + 32 * G::as;
    float* Xs = regions + (wave < a.n_waves ? wave : 0) * per_wave;
    float* As = Xs + as_off;
    float* Ds = Xs + ds_off;
    const int kb_features = (a.F + 31) >> 5;

    // the weight-gradient tiles this wave owns (backward): tile o of a layer belongs to wave o % 4
    constexpr int NT0 = (HB * KB1 + 3) / 4, NTM = (HB * HB + 3) / 4, NTO = (HB + 3) / 4;
    f32x16 gW0[NT0], gWm[NL > 2 ? NL - 2 : 1][NTM], gWo[NTO];
    float gb[NL];
    if constexpr (BWD) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
#pragma unroll
            for (int q = 0; q < NT0; ++q) gW0[q][r] = 0.f;
#pragma unroll
            for (int m = 0; m < NL - 2; ++m)
#pragma unroll
                for (int q = 0; q < NTM; ++q) gWm[m][q][r] = 0.f;
#pragma unroll
            for (int q = 0; q < NTO; ++q) gWo[q][r] = 0.f;
        }
#pragma unroll
        for (int l = 0; l < NL; ++l) gb[l] = 0.f;
    }

    for (int blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        // ---- compact the visible rows of the block
        const long long row_ll = (long long)blk * AP_BLOCK + tid;
        const bool in_range = row_ll < a.N;
        const int my_row = (int)row_ll;
        const bool vis = in_range && (a.mask == nullptr || a.mask[my_row] != 0);
        const unsigned long long ballot = __ballot(vis);
        if (lane == 0) wcnt[wave] = __popcll(ballot);
        visf[tid] = vis ? 1 : 0;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int c = wcnt[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (vis) idx[before + __popcll(ballot & ((1ull << lane) - 1ull))] = my_row;
        if constexpr (!BWD) {
            if (in_range && !vis)
                for (int c = 0; c < a.n_out; ++c) out[(size_t)my_row * a.n_out + c] = 0.f;
        }
        __syncthreads();
        if (want_f) {
            // rows the mask hides: their gradient rows are written as zeros, four floats at a time (F % 4 == 0)
            const int f4 = a.F >> 2;
            float4* dst = reinterpret_cast<float4*>(v_features + (size_t)blk * AP_BLOCK * a.F);
            for (int e = tid; e < AP_BLOCK * f4; e += AP_BLOCK) {
                const int r = e / f4;
                if ((long long)blk * AP_BLOCK + r < a.N && !visf[r]) dst[e] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }

        // ---- rounds of n_waves tiles; every wave walks every round (the weight gradient is the workgroup's work)
        const int tiles = (total + AP_TILE - 1) / AP_TILE;
        for (int t0 = 0; t0 < tiles; t0 += a.n_waves) {
            const int n_active = min(a.n_waves, tiles - t0);
            const bool active = wave < n_active;
            const int t = t0 + wave;
            const int cnt = active ? min(AP_TILE, total - t * AP_TILE) : 0;
            const bool valid = j < cnt;
            const int row = valid ? idx[t * AP_TILE + j] : 0;
            float norm = 1.f;
            f32x16 act[NL - 1][HB];
            float y[4];

            if (active) {
                // ---- the first layer's input, [row][k] in LDS: features (normalised), encoded direction, zero padding
                ap_wave_sync();
#pragma unroll 4
                for (int rr = 0; rr < AP_TILE; ++rr) {
                    const bool there = rr < cnt;
                    const size_t base = there ? (size_t)idx[t * AP_TILE + rr] * a.F : 0;
                    for (int k = lane; k < a.F; k += 64) Xs[rr * G::xs + k] = there ? a.features[base + k] : 0.f;
                }
                for (int k = a.K1 + h; k < 32 * KB1; k += 2) Xs[j * G::xs + k] = 0.f;
                if (a.P > 0) {
                    float d[3] = {0.f, 0.f, 0.f};
                    if (valid) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) d[c] = a.means[(size_t)row * 3 + c] - a.cam[c];
                        const float inv = 1.f / fmaxf(sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), 1e-12f);
#pragma unroll
                        for (int c = 0; c < 3; ++c) d[c] *= inv;
                    }
                    for (int p = h; p < a.P; p += 2) Xs[j * G::xs + a.F + p] = valid ? ap_encode(d, p) : 0.f;
                }
                ap_wave_sync();
                if (normalize) {
                    float ss = 0.f;
                    for (int k = h; k < a.F; k += 2) ss = fmaf(Xs[j * G::xs + k], Xs[j * G::xs + k], ss);
                    ss += __shfl_xor(ss, 32, 64);
                    norm = sqrtf(ss);
                    const float inv = 1.f / fmaxf(norm, 1e-12f);
                    for (int k = h; k < a.F; k += 2) Xs[j * G::xs + k] *= inv;
                    ap_wave_sync();
                }

                // ---- forward
                ap_dense_lds<HB, KB1>(ap_lds + G::w_off(0), G::stride(0), bias, Xs, G::xs, act[0], j, h);
                ap_relu<HB>(act[0]);
#pragma unroll
                for (int l = 1; l < NL - 1; ++l) {
                    ap_dense<HB, HB>(ap_lds + G::w_off(l), G::stride(l), bias + 64 * l, act[l - 1], act[l], j, h);
                    ap_relu<HB>(act[l]);
                }
                f32x16 z[1];
                ap_dense<1, HB>(ap_lds + G::w_off(NL - 1), G::stride(NL - 1), bias + 64 * (NL - 1), act[NL - 2], z, j, h);
#pragma unroll
                for (int c = 0; c < 4; ++c) y[c] = sigmoid ? 1.f / (1.f + expf(-z[0][c])) : z[0][c];
                if constexpr (!BWD) {
                    if (valid && h == 0) {
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            if (c < a.n_out) out[(size_t)row * a.n_out + c] = y[c];
                    }
                }
            }

            if constexpr (BWD) {
                // ---- backward: delta of the output layer (neurons 0 .. n_out-1 are registers 0 .. 3 of lane half 0)
                f32x16 dout[1];
#pragma unroll
                for (int r = 0; r < 16; ++r) dout[0][r] = 0.f;
                if (valid && h == 0) {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (c < a.n_out) {
                            const float g = v_out[(size_t)row * a.n_out + c];
                            dout[0][c] = sigmoid ? g * (y[c] * (1.f - y[c])) : g;
                        }
                }
                f32x16 d[HB];
                if (want_w) {
                    if (active) {
                        ap_put_delta<1>(Ds, dout, j, h);
                        ap_put_act<HB>(As, G::as, act[NL - 2], j, h);
                    }
                    __syncthreads();
                    ap_wgrad<1, HB>(regions, per_wave, ds_off, as_off, G::as, n_active, gWo, gb[NL - 1], wave, lane);
                    __syncthreads();
                }
                if (active) {
                    ap_dense_t<1, HB, 4>(ap_lds + G::w_off(NL - 1), G::stride(NL - 1), dout, d, HB, j, h);
                    ap_relu_bwd<HB>(d, act[NL - 2]);
                }
#pragma unroll
                for (int l = NL - 2; l >= 1; --l) {
                    if (want_w) {
                        if (active) {
                            ap_put_delta<HB>(Ds, d, j, h);
                            ap_put_act<HB>(As, G::as, act[l - 1], j, h);
                        }
                        __syncthreads();
                        ap_wgrad<HB, HB>(regions, per_wave, ds_off, as_off, G::as, n_active, gWm[l - 1], gb[l], wave, lane);
                        __syncthreads();
                    }
                    if (active) {
                        f32x16 dp[HB];
                        ap_dense_t<HB, HB, 16>(ap_lds + G::w_off(l), G::stride(l), d, dp, HB, j, h);
                        ap_relu_bwd<HB>(dp, act[l - 1]);
#pragma unroll
                        for (int kb = 0; kb < HB; ++kb) d[kb] = dp[kb];
                    }
                }
                if (want_w) {
                    if (active) ap_put_delta<HB>(Ds, d, j, h);
                    __syncthreads();
                    ap_wgrad<HB, KB1>(regions, per_wave, ds_off, 0, G::xs, n_active, gW0, gb[0], wave, lane);
                    __syncthreads();
                }
                if (want_f && active) {
                    float scale = 1.f, dot = 0.f;
                    if (normalize && norm < 1e-12f) scale = 1e12f;      // F.normalize: under eps the divisor is the constant
                    else if (normalize) scale = 1.f / norm;
                    constexpr int KBF = KB1 < 4 ? KB1 : 4;      // the feature columns end at 128
                    f32x16 g[KBF];
                    ap_dense_t<HB, KBF, 16>(ap_lds + G::w_off(0), G::stride(0), d, g, kb_features, j, h);
                    if (normalize && norm >= 1e-12f) {
#pragma unroll
                        for (int kb = 0; kb < KBF; ++kb)
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const int k = 32 * kb + ap_perm(r, h);
                                if (k < a.F) dot = fmaf(Xs[j * G::xs + k], g[kb][r], dot);
                            }
                    }
                    dot += __shfl_xor(dot, 32, 64);
#pragma unroll
                    for (int kb = 0; kb < KBF; ++kb)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int k0 = 32 * kb + 8 * q + 4 * h;
                            if (valid && k0 < a.F) {
                                float v[4];
#pragma unroll
                                for (int c = 0; c < 4; ++c) {
                                    v[c] = g[kb][4 * q + c];
                                    if (normalize) v[c] = (v[c] - Xs[j * G::xs + k0 + c] * dot) * scale;
                                }
                                *reinterpret_cast<float4*>(v_features + (size_t)row * a.F + k0) = make_float4(v[0], v[1], v[2], v[3]);
                            }
                        }
                }
                ap_wave_sync();
            }
        }
        __syncthreads();
    }

    if constexpr (BWD) {
        if (!want_w) return;
        // ---- one partial per workgroup, each tile written by the wave that owns it
        float* dst = partials + (size_t)blockIdx.x * ap_compact_total(a, NL);
        int off = 0;
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const int rows = ap_rows(a, l, NL), cols = ap_cols(a, l);
            if (l == 0) ap_dump<HB, KB1>(dst + off, rows, cols, gW0, wave, lane);
            else if (l == NL - 1) ap_dump<1, HB>(dst + off, rows, cols, gWo, wave, lane);
            else ap_dump<HB, HB>(dst + off, rows, cols, gWm[l - 1], wave, lane);
            off += rows * cols;
            if (wave == 0 && lane < rows) dst[off + lane] = gb[l];
            off += rows;
        }
    }
}

// Sums the workgroups' partials in workgroup order and writes the gradients in the parameters' own layout:
//   v_params = [W_0 [H, F + E + P] | b_0 | W_1 | b_1 | ... | embedding [E]]
// Block 0 owns what follows from the first bias: v_b0, v_W0[:, F:F+E] = v_b0 (x) e^, v_e^ = W_0[:, F:F+E]^T v_b0 and, with
// AP_NORMALIZE, the backward of F.normalize on the embedding.  The other blocks take one compact element per thread.
__global__ __launch_bounds__(256) void ap_reduce_kernel(ApNet a, int NL, int n_partials, const float* __restrict__ partials,
                                                        float* __restrict__ v_params) {
    const int total_p = ap_compact_total(a, NL);
    const int tid = threadIdx.x;
    if (blockIdx.x > 0) {
        const int e = (blockIdx.x - 1) * 256 + tid;
        if (e >= total_p) return;
        int coff = 0, toff = 0, dst = -1;
        for (int l = 0; l < NL; ++l) {
            const int rows = ap_rows(a, l, NL), cols = ap_cols(a, l), in = ap_in(a, l);
            if (e < coff + rows * cols) {
                const int i = (e - coff) / cols, k = (e - coff) - i * cols;
                dst = toff + i * in + ((l == 0 && k >= a.F) ? k + a.E : k);
                break;
            }
            coff += rows * cols;
            toff += rows * in;
            if (e < coff + rows) {
                dst = l == 0 ? -1 : toff + (e - coff);
                break;
            }
            coff += rows;
            toff += rows;
        }
        if (dst < 0) return;
        float sum = 0.f;
        for (int g = 0; g < n_partials; ++g) sum += partials[(size_t)g * total_p + e];
        v_params[dst] = sum;
        return;
    }
    __shared__ float vb[64], ehat[AP_MAX_E], ve[AP_MAX_E], stats[2];
    const int in0 = ap_in(a, 0), b0_compact = a.H * a.K1, b0_true = a.H * in0;
    int emb_true = 0;
    for (int l = 0; l < NL; ++l) emb_true += ap_rows(a, l, NL) * (ap_in(a, l) + 1);
    if (tid < a.H) {
        float sum = 0.f;
        for (int g = 0; g < n_partials; ++g) sum += partials[(size_t)g * total_p + b0_compact + tid];
        vb[tid] = sum;
        v_params[b0_true + tid] = sum;
    }
    for (int e = tid; e < a.E; e += 256) ehat[e] = a.emb[e];
    __syncthreads();
    if (tid == 0) {
        float ss = 0.f;
        for (int e = 0; e < a.E; ++e) ss = fmaf(ehat[e], ehat[e], ss);
        stats[0] = sqrtf(ss);
    }
    __syncthreads();
    const bool normalize = a.flags & AP_NORMALIZE;
    const float norm = stats[0];
    if (normalize)
        for (int e = tid; e < a.E; e += 256) ehat[e] *= 1.f / fmaxf(norm, 1e-12f);
    for (int e = tid; e < a.E; e += 256) {
        float sum = 0.f;
        for (int i = 0; i < a.H; ++i) sum = fmaf(a.W[0][(size_t)i * in0 + a.F + e], vb[i], sum);
        ve[e] = sum;
    }
    __syncthreads();
    for (int e = tid; e < a.H * a.E; e += 256) {
        const int i = e / a.E, c = e - i * a.E;
        v_params[(size_t)i * in0 + a.F + c] = vb[i] * ehat[c];
    }
    if (tid == 0) {
        float dot = 0.f;
        for (int e = 0; e < a.E; ++e) dot = fmaf(ehat[e], ve[e], dot);
        stats[1] = dot;
    }
    __syncthreads();
    for (int e = tid; e < a.E; e += 256) {
        float v = ve[e];
        if (normalize) v = norm >= 1e-12f ? (v - ehat[e] * stats[1]) / norm : v * 1e12f;
        v_params[emb_true + e] = v;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
static int ap_fill(const char* who, ApNet& a, int& NL, int N, int F, int E, int H, int n_layers, int n_out, int n_freq, int flags,
                   const float* features, const uint8_t* mask, const float* means, const float* camera_center, const float* embedding,
                   const float* const* weights, const float* const* biases) {
    if (N < 0 || N > 0x7fffffff - AP_BLOCK) return fail_arg(who);
    if (F < 4 || F > 128 || F % 4) { set_error(who, "n_features must be a multiple of 4 in 4 .. 128"); return GSPL_ERR_INVALID_ARG; }
    if (E < 0 || E > AP_MAX_E) { set_error(who, "n_embedding_dims must be 0 .. 256"); return GSPL_ERR_INVALID_ARG; }
    if (H != 32 && H != 64) { set_error(who, "n_neurons must be 32 or 64"); return GSPL_ERR_INVALID_ARG; }
    if (n_layers < 2 || n_layers > AP_MAX_LAYERS) { set_error(who, "n_layers must be 2 .. 4"); return GSPL_ERR_INVALID_ARG; }
    if (n_out != 3 && n_out != 4) { set_error(who, "n_out must be 3 or 4"); return GSPL_ERR_INVALID_ARG; }
    if (n_freq < 0 || n_freq > 8) { set_error(who, "n_view_frequencies must be 0 .. 8"); return GSPL_ERR_INVALID_ARG; }
    if (flags & ~(AP_NORMALIZE | AP_SIGMOID)) return fail_arg(who);
    if (!weights || !biases) return fail_arg(who);
    NL = n_layers;
    a = ApNet{};
    a.N = N; a.F = F; a.E = E; a.H = H; a.n_out = n_out; a.n_freq = n_freq; a.flags = flags;
    a.P = n_freq > 0 ? 3 * (2 * n_freq + 1) : 0;
    a.K1 = F + a.P;
    a.n_blocks = (N + AP_BLOCK - 1) / AP_BLOCK;
    a.features = features; a.mask = mask; a.means = means; a.cam = camera_center; a.emb = embedding;
    for (int l = 0; l < n_layers; ++l) {
        if (!weights[l] || !biases[l]) return fail_arg(who);
        a.W[l] = weights[l];
        a.B[l] = biases[l];
    }
    if (N > 0 && (!features || (E > 0 && !embedding) || (a.P > 0 && (!means || !camera_center)))) return fail_arg(who);
    if ((a.K1 + 31) / 32 > AP_MAX_KB1) { set_error(who, "first layer too wide"); return GSPL_ERR_INVALID_ARG; }
    return GSPL_OK;
}

template <int KB1, int HB, int NL>
static int ap_waves(bool bwd) {
    for (int w = 4; w >= 1; w >>= 1)
        if ((size_t)ApGeom<KB1, HB, NL>::total(bwd, w) * sizeof(float) <= (size_t)AP_LDS_BYTES) return w;
    return 0;
}

template <int KB1, int HB, int NL, bool BWD>
static int ap_launch(ApNet a, int grid, float* out, const float* v_out, float* v_features, float* partials, hipStream_t s, const char* who) {
    a.n_waves = ap_waves<KB1, HB, NL>(BWD);
    if (a.n_waves == 0) { set_error(who, "the network does not fit the LDS budget"); return GSPL_ERR_INVALID_ARG; }
    const size_t lds_bytes = (size_t)ApGeom<KB1, HB, NL>::total(BWD, a.n_waves) * sizeof(float);
    if (lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ap_kernel<KB1, HB, NL, BWD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return check_hip(e, who);
    }
    hipLaunchKernelGGL((ap_kernel<KB1, HB, NL, BWD>), dim3(grid), dim3(AP_BLOCK), lds_bytes, s, a, out, v_out, v_features, partials);
    return check_launch(who);
}

template <bool BWD, class... Args>
static int ap_dispatch(const ApNet& a, int NL, Args... args) {
    const int KB1 = (a.K1 + 31) / 32, HB = a.H / 32;
#define AP_CASE(K, H, L) if (KB1 == K && HB == H && NL == L) return ap_launch<K, H, L, BWD>(a, args...);
#define AP_CASES(K) AP_CASE(K, 1, 2) AP_CASE(K, 1, 3) AP_CASE(K, 1, 4) AP_CASE(K, 2, 2) AP_CASE(K, 2, 3) AP_CASE(K, 2, 4)
    AP_CASES(1) AP_CASES(2) AP_CASES(3) AP_CASES(4) AP_CASES(5) AP_CASES(6)
#undef AP_CASES
#undef AP_CASE
    return GSPL_ERR_INVALID_ARG;
}

static int ap_grid(const ApNet& a) { return a.n_blocks < AP_GRID ? a.n_blocks : AP_GRID; }
static size_t ap_true_total(const ApNet& a, int NL) {
    size_t o = a.E;
    for (int l = 0; l < NL; ++l) o += (size_t)ap_rows(a, l, NL) * (ap_in(a, l) + 1);
    return o;
}

}  // namespace gspl

using namespace gspl;

extern "C" size_t gspl_appearance_mlp_workspace_bytes(int N, int F, int E, int H, int n_layers, int n_out, int n_freq) {
    ApNet a{};
    a.N = N; a.F = F; a.E = E; a.H = H; a.n_out = n_out;
    a.P = n_freq > 0 ? 3 * (2 * n_freq + 1) : 0;
    a.K1 = F + a.P;
    a.n_blocks = N > 0 ? (N + AP_BLOCK - 1) / AP_BLOCK : 0;
    return up256((size_t)(ap_grid(a) > 0 ? ap_grid(a) : 1) * ap_compact_total(a, n_layers) * sizeof(float));
}

extern "C" int gspl_appearance_mlp_fwd(int N, int F, int E, int H, int n_layers, int n_out, int n_freq, int flags, const float* features,
                                       const uint8_t* mask, const float* means, const float* camera_center, const float* embedding,
                                       const float* const* weights, const float* const* biases, float* out, void* stream) {
    ApNet a;
    int NL;
    if (const int rc = ap_fill("gspl_appearance_mlp_fwd", a, NL, N, F, E, H, n_layers, n_out, n_freq, flags, features, mask, means, camera_center,
                               embedding, weights, biases)) return rc;
    if (N == 0) return GSPL_OK;
    if (!out) return fail_arg("gspl_appearance_mlp_fwd");
    return ap_dispatch<false>(a, NL, ap_grid(a), out, (const float*)nullptr, (float*)nullptr, (float*)nullptr, (hipStream_t)stream, "gspl_appearance_mlp_fwd");
}

extern "C" int gspl_appearance_mlp_bwd(int N, int F, int E, int H, int n_layers, int n_out, int n_freq, int flags, const float* features,
                                       const uint8_t* mask, const float* means, const float* camera_center, const float* embedding,
                                       const float* const* weights, const float* const* biases, const float* v_out, float* v_features,
                                       float* v_params, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "gspl_appearance_mlp_bwd";
    ApNet a;
    int NL;
    if (const int rc = ap_fill(who, a, NL, N, F, E, H, n_layers, n_out, n_freq, flags, features, mask, means, camera_center, embedding,
                               weights, biases)) return rc;
    if (!v_features && !v_params) return GSPL_OK;
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {
        if (v_params) return check_hip(hipMemsetAsync(v_params, 0, ap_true_total(a, NL) * sizeof(float), s), who);
        return GSPL_OK;
    }
    if (!v_out) return fail_arg(who);
    if (v_features && ((uintptr_t)v_features & 15)) { set_error(who, "v_features must be aligned to 16 bytes"); return GSPL_ERR_INVALID_ARG; }
    const int grid = ap_grid(a);
    if (v_params) {
        if (!workspace) return fail_arg(who);
        if (workspace_bytes < (size_t)grid * ap_compact_total(a, NL) * sizeof(float)) return fail_ws(who);
    }
    if (const int rc = ap_dispatch<true>(a, NL, grid, (float*)nullptr, v_out, v_features, v_params ? (float*)workspace : (float*)nullptr, s, who)) return rc;
    if (v_params) {
        const int blocks = 1 + (ap_compact_total(a, NL) + 255) / 256;
        hipLaunchKernelGGL(ap_reduce_kernel, dim3(blocks), dim3(256), 0, s, a, NL, grid, (const float*)workspace, v_params);
        return check_launch("gspl_appearance_mlp_bwd (reduce)");
    }
    return GSPL_OK;
}

// features.hip — wide-feature alpha compositing: forward, and a backward that yields the feature gradient ONLY (gfx950, wave64);
// include/gspl_hip.h section 16.
//
// Feature-3DGS (internal/renderers/feature_3dgs_renderer.py: 128 / 256 / 512 channels per splat) and SegAnyGS
// (internal/renderers/gsplat_contrastive_feature_renderer.py: 32) composite many channels over a FROZEN model: the blending weights
// alpha T do not depend on the channel and no geometry gradient is asked for.  The kernels of composite.hip are built for D <= 8 and a
// backward that reduces 6 + D values per (tile, splat); here the cost per channel is one multiply-add per (pixel, splat):
//   * feature_fwd_kernel: the 8x8 block walk of gspl_composite.h (one wave per 8x8 block, lane = pixel, rounds of 64 list entries compacted
//     into LDS: walk_block, compact_round, pixel_alpha, blend_step — the definitions composite_fwd_kernel takes its decisions with), CH
//     channels in registers per workgroup, the chunks of CH on grid.y.  Every chunk re-evaluates the weights (~20 VALU instructions per
//     candidate against CH multiply-adds); chunk 0 writes alpha, T and last_ids.  Per channel the sum is the fmaf chain of
//     composite_fwd_kernel in list order: the image is bit-for-bit the one the narrow kernels give channel by channel.  What is this
//     kernel's own: the list position and splat id staged beside the round's common arrays, the feature rows, the channel sums.
//   * feature_bwd_kernel: v_features[g, c] += sum_pixels (alpha T) v_out[pixel, c].  The same walk front to back up to last_ids, T
//     recomputed with the forward's expressions (pixel_alpha; alpha_test behind "not behind this pixel's last contributor").  The sum over the block's 64 pixels is a TRANSPOSE, not a cross-lane reduction: phase 1 (lane = pixel)
//     leaves the round's weights W[candidate][pixel] in LDS; phase 2 (lane = channel) holds its channel's 64 v_out values in registers
//     and accumulates sum_p W[k][p] v[p], W arriving as LDS broadcasts (one ds_read_b128 per four multiply-adds).  Lane c then owns
//     (k, c): one fp32 atomic per (block, splat, channel), 64 consecutive channels of one splat row per instruction.  Up to 32 channels
//     the wave splits the pixels instead: lane = (pixel half, channel), 32 multiply-adds each and one cross-half add.
// Resource use: profiles/feature_kernel_resources.txt.
#include "gspl_composite.h"

namespace gspl {
namespace {

constexpr int kRound = 64;               // list entries per round = lanes
constexpr int kWStride = 64;             // W[candidate][pixel]: rows of 64 floats (16-byte aligned reads of four pixels)
constexpr int kVStride = 65;             // the CHW staging of v_out, [channel][pixel]: odd stride, lane = channel reads hit 64 banks

// acc + T bg as the narrow kernels round it.  composite_fwd_kernel writes `acc[c] + T * bgc`, and what hipcc makes of it is part of
// the bits its callers see: in every instantiation (D = 1, 2, 3, 4, 8; both modes and layouts) the channels are finished in pairs, the
// even one by a fused multiply-add, the odd one by a rounded product and an add.  The channel adapter cuts on multiples of 8, so the
// parity is the channel's own.  Spelled out here (contraction off) so that the image stays bit-for-bit the narrow kernels' whatever the
// compiler would make of the plain expression in THIS kernel; tests/test_features_gpu.py compares the two with a random background.
__device__ __forceinline__ float add_background(float acc, float T, float bg, bool even_channel) {
#pragma clang fp contract(off)
    const float product = T * bg;
    return even_channel ? fmaf(T, bg, acc) : acc + product;
}

template <int CH, int MODE, bool CHW>
__global__ __launch_bounds__(64) void feature_fwd_kernel(
    int n_tiles, int tile_w, int width, int height, int64_t n_isects, int D, bool empty,
    const float* __restrict__ means2d, const float* __restrict__ conics, const float* __restrict__ features,
    const float* __restrict__ opacities, const float* __restrict__ backgrounds,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ flatten_ids,
    float* __restrict__ out, float* __restrict__ out_alphas, float* __restrict__ final_Ts, int32_t* __restrict__ last_ids, ListTiles lt) {
    __shared__ RoundLists s;
    __shared__ int s_pos[kRound], s_g[kRound];      // list index + 1 and splat of each candidate
    __shared__ __attribute__((aligned(16))) float s_f[kRound * CH];      // [candidate][channel of the chunk], zero beyond D
    const int l = threadIdx.x, c0 = blockIdx.y * CH;
    const WalkBlock b = walk_block<MODE>(xcd_remap(blockIdx.x, 4 * n_tiles, 4 * GSPL_XCD_RUN), tile_w);
    const bool inside = (b.px < width) && (b.py < height);
    int start = 0, end = 0;      // (`empty`: no list exists — N == 0 or no intersections — and `offsets` is not read)
    if (!empty) block_list_range(lt, b.bx, b.by, width, height, n_isects, offsets, start, end);

    float T = 1.f;
    float acc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = 0.f;
    int last = start;
    bool done = !inside;

    if (!__all(done)) {
        int g_next = (start + l < end) ? flatten_ids[start + l] : 0;
        for (int base = start; base < end; base += kRound) {
            const int g = g_next;
            if (base + kRound + l < end) g_next = flatten_ids[base + kRound + l];
            const RoundSlot r = compact_round(base + l < end, g, means2d, conics, opacities, b, s);
            if (r.cand) { s_pos[r.slot] = base + l + 1; s_g[r.slot] = g; }
            __builtin_amdgcn_wave_barrier();
            const int ncand = r.ncand;
            if (ncand == 0) continue;
            // the candidates' feature rows: 64 lanes read consecutive channels of one row (two rows with CH == 32)
            for (int e = l; e < ncand * CH; e += 64) {
                const int k = e / CH, c = c0 + (e % CH);
                s_f[e] = c < D ? features[(int64_t)s_g[k] * D + c] : 0.f;
            }
            __builtin_amdgcn_wave_barrier();
            bool all_done = false;
            for (int k = 0; k < ncand; ++k) {
                const PixelAlpha pa = pixel_alpha(s, k, b.pxf, b.pyf);
                float wgt;
                const bool contrib = blend_step<MODE>(pa.sigma, clamp_alpha<MODE>(pa.raw), T, done, wgt);
#pragma unroll
                for (int c = 0; c < CH; c += 4) {
                    const float4 f = *reinterpret_cast<const float4*>(&s_f[k * CH + c]);
                    acc[c + 0] = fmaf(f.x, wgt, acc[c + 0]);
                    acc[c + 1] = fmaf(f.y, wgt, acc[c + 1]);
                    acc[c + 2] = fmaf(f.z, wgt, acc[c + 2]);
                    acc[c + 3] = fmaf(f.w, wgt, acc[c + 3]);
                }
                last = contrib ? s_pos[k] : last;
                if (__all(done)) { all_done = true; break; }
            }
            if (all_done) break;
        }
    }

    if (inside) {
        const int64_t pix = (int64_t)b.py * width + b.px, P = (int64_t)width * height;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            if (c0 + c < D) {
                const float bgc = backgrounds ? backgrounds[c0 + c] : 0.f;
                const float v = add_background(acc[c], T, bgc, (c & 1) == 0);      // (c0 is even)
                if (CHW) out[(int64_t)(c0 + c) * P + pix] = v;
                else out[pix * D + c0 + c] = v;
            }
        }
        if (blockIdx.y == 0) {
            out_alphas[pix] = 1.f - T;
            final_Ts[pix] = T;
            last_ids[pix] = last;
        }
    }
}

// HALF: D <= 32 — lane = (pixel half, channel): 32 channels per workgroup, 32 pixels per lane.
template <int MODE, bool CHW, bool HALF>
__global__ __launch_bounds__(64) void feature_bwd_kernel(
    int n_tiles, int tile_w, int width, int height, int64_t n_isects, int D,
    const float* __restrict__ means2d, const float* __restrict__ conics, const float* __restrict__ opacities,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ flatten_ids, const int32_t* __restrict__ last_ids,
    const float* __restrict__ v_out, float* __restrict__ v_features, ListTiles lt) {
    constexpr int LC = HALF ? 32 : 64;        // channels per workgroup
    constexpr int PXL = HALF ? 32 : 64;       // pixels per lane in phase 2
    __shared__ RoundLists s;
    __shared__ int s_pos[kRound], s_g[kRound];      // list index + 1 and splat of each candidate
    __shared__ __attribute__((aligned(16))) float s_w[64 * kVStride];
    const int l = threadIdx.x, c0 = blockIdx.y * LC;
    const WalkBlock b = walk_block<MODE>(xcd_remap(blockIdx.x, 4 * n_tiles, 4 * GSPL_XCD_RUN), tile_w);
    const bool inside = (b.px < width) && (b.py < height);
    int start, end;
    block_list_range(lt, b.bx, b.by, width, height, n_isects, offsets, start, end);

    // this pixel's walk ends behind its last contributing entry; the wave's behind the latest of them
    const int64_t P = (int64_t)width * height;
    const int last = inside ? last_ids[(int64_t)b.py * width + b.px] : 0;
    int wave_last = last;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) wave_last = max(wave_last, __shfl_xor(wave_last, off));
    end = min(end, wave_last);
    if (end <= start) return;

    // phase 2's registers: v[j] = v_out[pixel p0 + j of the block, channel cl]; zero outside the image and beyond D
    const int cl = c0 + (l % LC), p0 = HALF ? (l >> 5) * 32 : 0;
    const int bx0 = b.px - (l & 7), by0 = b.py - (l >> 3);
    float v[PXL];
    if (CHW) {
        // planes: read with lane = pixel (rows of eight pixels), turn through LDS
        for (int c = 0; c < LC; ++c)
            s_w[c * kVStride + l] = (inside && c0 + c < D) ? v_out[(int64_t)(c0 + c) * P + (int64_t)b.py * width + b.px] : 0.f;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < PXL; ++j) v[j] = s_w[(l % LC) * kVStride + p0 + j];
        __builtin_amdgcn_wave_barrier();
    } else {
#pragma unroll
        for (int j = 0; j < PXL; ++j) {
            const int p = p0 + j, qx = bx0 + (p & 7), qy = by0 + (p >> 3);
            v[j] = (qx < width && qy < height && cl < D) ? v_out[((int64_t)qy * width + qx) * D + cl] : 0.f;
        }
    }

    float T = 1.f;
    int g_next = (start + l < end) ? flatten_ids[start + l] : 0;
    for (int base = start; base < end; base += kRound) {
        const int g = g_next;
        if (base + kRound + l < end) g_next = flatten_ids[base + kRound + l];
        const RoundSlot r = compact_round(base + l < end, g, means2d, conics, opacities, b, s);
        if (r.cand) { s_pos[r.slot] = base + l + 1; s_g[r.slot] = g; }
        __builtin_amdgcn_wave_barrier();
        const int ncand = r.ncand;
        if (ncand == 0) continue;
        // phase 1, lane = pixel: the weights of the round; bit k of `hit` = some pixel blended candidate k
        unsigned long long hit = 0ull;
        for (int k = 0; k < ncand; ++k) {
            const PixelAlpha pa = pixel_alpha(s, k, b.pxf, b.pyf);
            const float alpha = clamp_alpha<MODE>(pa.raw);
            // every entry in front of `last` that passed the forward's test was blended there (the stop comes behind `last`)
            const bool contrib = alpha_test(s_pos[k] <= last, pa.sigma, alpha);
            s_w[k * kWStride + l] = contrib ? alpha * T : 0.f;
            T = contrib ? T * (1.f - alpha) : T;
            hit |= (__ballot(contrib) != 0ull ? 1ull : 0ull) << k;
        }
        __builtin_amdgcn_wave_barrier();
        // phase 2, lane = channel: sum over the pixels, W as broadcasts
        while (hit) {
            const int k = __builtin_ctzll(hit);
            hit &= hit - 1ull;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
            for (int j = 0; j < PXL; j += 4) {
                const float4 w4 = *reinterpret_cast<const float4*>(&s_w[k * kWStride + p0 + j]);
                a0 = fmaf(w4.x, v[j + 0], a0);
                a1 = fmaf(w4.y, v[j + 1], a1);
                a2 = fmaf(w4.z, v[j + 2], a2);
                a3 = fmaf(w4.w, v[j + 3], a3);
            }
            float a = (a0 + a1) + (a2 + a3);
            if (HALF) a += __shfl_xor(a, 32);
            if (l < LC && cl < D) atomicAdd(v_features + (int64_t)s_g[k] * D + cl, a);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace

static int check_feature_args(int N, int64_t n_isects, int D, int mode, int layout, ImageSize image, TileGrid grid, const char* who) {
    if (D < 1) return fail_arg(who);
    // everything but the channel count is the compositing calls' own check
    return check_composite_args(N, n_isects, 1, mode, layout, image, grid, who);
}

}  // namespace gspl

extern "C" int gspl_feature_fwd(int N, int64_t n_isects, int D, int mode, int layout,
                                const float* means2d, const float* conics, const float* features, const float* opacities,
                                const float* backgrounds, int width, int height, int tile_size, int tile_w, int tile_h,
                                const int32_t* offsets, const int32_t* flatten_ids,
                                float* out, float* out_alphas, float* final_Ts, int32_t* last_ids, void* stream) {
    using namespace gspl;
    const ImageSize image{width, height};
    const TileGrid grid{tile_size, tile_w, tile_h};
    const int rc = check_feature_args(N, n_isects, D, mode, layout, image, grid, "feature_fwd: bad argument");
    if (rc != GSPL_OK) return rc;
    if (!out || !out_alphas || !final_Ts || !last_ids) return fail_arg("feature_fwd: NULL required pointer");
    const bool empty = N == 0 || n_isects == 0;
    if (!empty && (!means2d || !conics || !features || !opacities || !offsets || !flatten_ids)) return fail_arg("feature_fwd: NULL required pointer");
    const ListTiles lt = list_tiles(grid);
    const ComputeTiles ct = compute_tiles(image);
    hipStream_t s = (hipStream_t)stream;
    auto launch = [&](auto ch, auto inria, auto chw) {
        constexpr int CH = decltype(ch)::value;
        constexpr int MODE = decltype(inria)::value ? GSPL_MODE_INRIA : GSPL_MODE_GSPLAT;
        const int chunks = (D + CH - 1) / CH;
        if (chunks > 65535) return fail_arg("feature_fwd: D too large");
        hipLaunchKernelGGL((feature_fwd_kernel<CH, MODE, decltype(chw)::value>), dim3(4 * ct.n, chunks), dim3(64), 0, s,
                           ct.n, ct.w, width, height, n_isects, D, empty, means2d, conics, features, opacities, backgrounds, offsets, flatten_ids,
                           out, out_alphas, final_Ts, last_ids, lt);
        return check_launch("feature_fwd");
    };
    return dispatch_bools([&](auto wide, auto inria, auto chw) {
        if constexpr (decltype(wide)::value) return launch(std::integral_constant<int, 64>{}, inria, chw);
        else return launch(std::integral_constant<int, 32>{}, inria, chw);
    }, D > 32, mode != GSPL_MODE_GSPLAT, layout != GSPL_LAYOUT_HWC);
}

extern "C" int gspl_feature_bwd(int N, int64_t n_isects, int D, int mode, int layout,
                                const float* means2d, const float* conics, const float* opacities,
                                int width, int height, int tile_size, int tile_w, int tile_h,
                                const int32_t* offsets, const int32_t* flatten_ids, const int32_t* last_ids,
                                const float* v_out, float* v_features, void* stream) {
    using namespace gspl;
    const ImageSize image{width, height};
    const TileGrid grid{tile_size, tile_w, tile_h};
    const int rc = check_feature_args(N, n_isects, D, mode, layout, image, grid, "feature_bwd: bad argument");
    if (rc != GSPL_OK) return rc;
    if (N == 0 || n_isects == 0) return GSPL_OK;      // nothing was blended: v_features stays as the caller zeroed it
    if (!means2d || !conics || !opacities || !offsets || !flatten_ids || !last_ids || !v_out || !v_features) return fail_arg("feature_bwd: NULL required pointer");
    const ListTiles lt = list_tiles(grid);
    const ComputeTiles ct = compute_tiles(image);
    const bool half = D <= 32;
    const int chunks = half ? 1 : (D + 63) / 64;
    if (chunks > 65535) return fail_arg("feature_bwd: D too large");
    hipStream_t s = (hipStream_t)stream;
    return dispatch_bools([&](auto inria, auto chw, auto hf) {
        constexpr int MODE = decltype(inria)::value ? GSPL_MODE_INRIA : GSPL_MODE_GSPLAT;
        hipLaunchKernelGGL((feature_bwd_kernel<MODE, decltype(chw)::value, decltype(hf)::value>), dim3(4 * ct.n, chunks), dim3(64), 0, s,
                           ct.n, ct.w, width, height, n_isects, D, means2d, conics, opacities, offsets, flatten_ids, last_ids, v_out, v_features, lt);
        return check_launch("feature_bwd");
    }, mode != GSPL_MODE_GSPLAT, layout != GSPL_LAYOUT_HWC, half);
}

// bilagrid.hip — bilateral-grid slicing and its total-variation loss (gfx950, wave64); include/gspl_hip.h section 14.
//
// Wang et al., "Bilateral Guided Radiance Field Processing" (SIGGRAPH 2024): one affine colour transform per pixel, sliced out of a
// per-image grid G [12, L, GH, GW] at (x, y, gray(rgb)).  The reference's output processor (internal/output_processors/bilagrid.py)
// calls the CUDA package `fused_bilagrid` for it; its semantics are lib_bilagrid's `F.grid_sample(align_corners=True,
// padding_mode='border')` followed by the affine (header section 14 states them).
//   * slice_fwd_kernel: one thread per pixel, 96 gathers of the image's grid (L2-resident: 96 KiB at the default size).
//   * slice_bwd_rgb_kernel: the colour gradient, one thread per pixel (the same gathers plus the one-sided w difference).
//   * the grid gradient, deterministic and without float atomics: slice_bwd_blocks_kernel gives each square pixel block (side 64 << k)
//     ONE workgroup that owns the block's vertex window and sums the block's pixels into it in a fixed order (tent weight x the 12
//     per-pixel terms, in registers); it writes the window to the block's slab row and its extent to the block table.
//     slice_bwd_sum_kernel then gives every element of the dense gradient [N, 12, L, GH, GW] one thread that adds the slab rows
//     covering it, in block order, and writes 0 where no image of the batch selects the grid.
//   * tv_partials_kernel + tv_final_kernel: the TV loss as a fixed two-level sum; tv_bwd_kernel: its three-point stencil.
#include "gspl_device.h"
#include "gspl_host.h"
#include "gspl_reduce.h"

namespace gspl {
namespace {

constexpr int kT = 256;                 // threads per workgroup, every kernel
constexpr int kMaxL = 28;               // the 9 L owners of a 3 x 3 vertex tile fit one workgroup
constexpr int kMaxXY = 1024;            // GW, GH (10-bit fields of the staged pixel records)
constexpr int kMaxVertices = 16384;     // L GH GW: a slab row holds 12 of them (768 KiB at the bound)
constexpr int kMinBlock = 64;           // pixel block side: 64 << k
constexpr int kMaxBlocksPerImage = 512;
constexpr size_t kSlabBytesPerImage = (size_t)64 << 20;
constexpr int kTvMaxPartials = 1024;
constexpr int kTvPerPartial = 16384;

struct Geo {
    int L, GH, GW;
    int64_t LHW;                        // floats per channel of one grid
};

struct Img {
    int B, H, W;
    const float* xy;                    // [B or 1, H, W, 2]
    int64_t xy_bstride;                 // 0: one xy for every image
};

// channel c of pixel p of image b in a layout: HWC (interleaved) or CHW (planar); both have the image stride 3 H W
__device__ inline int64_t at(int layout, int b, int64_t P, int64_t p, int c) {
    return (int64_t)b * 3 * P + (layout == GSPL_LAYOUT_HWC ? p * 3 + c : (int64_t)c * P + p);
}

// grid_sample's unnormalisation (align_corners) and border clamp; wgrad: w strictly inside (0, L - 1), where d out / d w is not 0
struct Coords {
    int x0, y0, z0;
    float fx, fy, fz;
    bool wgrad;
};

__device__ inline double clampc(double c, int size) { return fmin(fmax(c, 0.0), (double)(size - 1)); }   // NaN -> 0

// The coordinates in fp64 (u = x (GW - 1), v = y (GH - 1), w = gray (L - 1): grid_sample's ((2x - 1) + 1) / 2 (size - 1) without its
// roundings): in fp32 they alone would move a sample by ~|dG| 1e-6; only the cell fractions are rounded to fp32.
__device__ inline Coords coords(float x, float y, float r, float g, float b, const Geo& G) {
    const double gray = 0.299 * (double)r + 0.587 * (double)g + 0.114 * (double)b;
    const double u = clampc((double)x * (G.GW - 1), G.GW);
    const double v = clampc((double)y * (G.GH - 1), G.GH);
    const double wr = gray * (G.L - 1);
    const double w = clampc(wr, G.L);
    Coords c;
    c.x0 = (int)floor(u);
    c.y0 = (int)floor(v);
    c.z0 = (int)floor(w);
    c.fx = (float)(u - c.x0);
    c.fy = (float)(v - c.y0);
    c.fz = (float)(w - c.z0);
    c.wgrad = wr > 0.0 && wr < (double)(G.L - 1);
    return c;
}

__device__ inline void uv_cell(float x, float y, const Geo& G, int& cx, int& cy) {
    cx = (int)floor(clampc((double)x * (G.GW - 1), G.GW));
    cy = (int)floor(clampc((double)y * (G.GH - 1), G.GH));
}

// A[k] (the trilinear sample) and, when D != nullptr, D[k] = B_k(z0 + 1) - B_k(z0) (d A / d w across the floor cell).  A corner past
// the last vertex is clamped onto it: its weight (the fraction) is exactly 0 there, so no read leaves the grid.
__device__ inline void sample(const float* __restrict__ g, const Geo& G, const Coords& c, float A[12], float* D) {
    const int x1 = min(c.x0 + 1, G.GW - 1), y1 = min(c.y0 + 1, G.GH - 1), z1 = min(c.z0 + 1, G.L - 1);
    const int64_t HW = (int64_t)G.GH * G.GW;
    const int64_t r00 = (int64_t)c.y0 * G.GW, r10 = (int64_t)y1 * G.GW;
    const int64_t p0 = (int64_t)c.z0 * HW, p1 = (int64_t)z1 * HW;
    const float w00 = (1.f - c.fy) * (1.f - c.fx), w01 = (1.f - c.fy) * c.fx, w10 = c.fy * (1.f - c.fx), w11 = c.fy * c.fx;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const float* q = g + (int64_t)k * G.LHW;
        const float b0 = w00 * q[p0 + r00 + c.x0] + w01 * q[p0 + r00 + x1] + w10 * q[p0 + r10 + c.x0] + w11 * q[p0 + r10 + x1];
        const float b1 = w00 * q[p1 + r00 + c.x0] + w01 * q[p1 + r00 + x1] + w10 * q[p1 + r10 + c.x0] + w11 * q[p1 + r10 + x1];
        A[k] = (1.f - c.fz) * b0 + c.fz * b1;
        if (D) D[k] = b1 - b0;
    }
}

__device__ inline int grid_of(const int32_t* __restrict__ idx, int idx_stride, int b, int N) {
    const int g = idx[(int64_t)b * idx_stride];
    return (g >= 0 && g < N) ? g : -1;
}

// ---- slice forward -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void slice_fwd_kernel(int N, Geo G, Img I, const float* __restrict__ grids, const float* __restrict__ rgb,
                                                       int layout, const int32_t* __restrict__ idx, int idx_stride, float* __restrict__ out) {
    const int64_t P = (int64_t)I.H * I.W;
    const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= P) return;
    const int g = grid_of(idx, idx_stride, b, N);
    if (g < 0) {
        const float nan = __int_as_float(0x7fc00000);
        for (int i = 0; i < 3; ++i) out[at(layout, b, P, p, i)] = nan;
        return;
    }
    const float r = rgb[at(layout, b, P, p, 0)], gg = rgb[at(layout, b, P, p, 1)], bb = rgb[at(layout, b, P, p, 2)];
    const float* xy = I.xy + b * I.xy_bstride + p * 2;
    const Coords c = coords(xy[0], xy[1], r, gg, bb, G);
    float A[12];
    sample(grids + (int64_t)g * 12 * G.LHW, G, c, A, nullptr);
#pragma unroll
    for (int i = 0; i < 3; ++i) out[at(layout, b, P, p, i)] = A[4 * i] * r + A[4 * i + 1] * gg + A[4 * i + 2] * bb + A[4 * i + 3];
}

// ---- slice backward: colour gradient -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void slice_bwd_rgb_kernel(int N, Geo G, Img I, const float* __restrict__ grids, const float* __restrict__ rgb,
                                                           int layout, const int32_t* __restrict__ idx, int idx_stride,
                                                           const float* __restrict__ grad_out, int go_layout, float* __restrict__ grad_rgb,
                                                           int gr_layout) {
    const int64_t P = (int64_t)I.H * I.W;
    const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= P) return;
    const int g = grid_of(idx, idx_stride, b, N);
    if (g < 0) {
        const float nan = __int_as_float(0x7fc00000);
        for (int j = 0; j < 3; ++j) grad_rgb[at(gr_layout, b, P, p, j)] = nan;
        return;
    }
    const float c3[3] = {rgb[at(layout, b, P, p, 0)], rgb[at(layout, b, P, p, 1)], rgb[at(layout, b, P, p, 2)]};
    const float d3[3] = {grad_out[at(go_layout, b, P, p, 0)], grad_out[at(go_layout, b, P, p, 1)], grad_out[at(go_layout, b, P, p, 2)]};
    const float* xy = I.xy + b * I.xy_bstride + p * 2;
    const Coords c = coords(xy[0], xy[1], c3[0], c3[1], c3[2], G);
    float A[12], D[12];
    sample(grids + (int64_t)g * 12 * G.LHW, G, c, A, D);
    float dw = 0.f;                                 // sum_k dA_k dA_k/dw
#pragma unroll
    for (int i = 0; i < 3; ++i) dw += d3[i] * (D[4 * i] * c3[0] + D[4 * i + 1] * c3[1] + D[4 * i + 2] * c3[2] + D[4 * i + 3]);
    dw = c.wgrad ? dw * (float)(G.L - 1) : 0.f;
    const float wgt[3] = {0.299f, 0.587f, 0.114f};
#pragma unroll
    for (int j = 0; j < 3; ++j)
        grad_rgb[at(gr_layout, b, P, p, j)] = d3[0] * A[j] + d3[1] * A[4 + j] + d3[2] * A[8 + j] + wgt[j] * dw;
}

// ---- slice backward: grid gradient, pass 1 (one workgroup per pixel block) ---------------------------------------------------------
// Block table entry (int4): x = the grid of the block's image (-1: invalid index, nothing written), y = vx0 | vx1 << 16, z = vy0 | vy1 << 16:
// the inclusive vertex window its pixels touch.  The slab row of a block is a full [12, L, GH, GW] image of which exactly the window is
// written.  The window is covered by 3 x 3-vertex tiles; for each tile, thread o < 9 L owns vertex o / L and level o % L, all 12
// channels, of pixel subset s = t / (9 L) (nsub = 256 / (9 L) subsets: pixels j = s, s + nsub, ... of each staged chunk of 256).
// Coherent images (xy a meshgrid) touch one tile per block at the default sizes; any xy still gets the exact sum, tile after tile.
struct BlockShape { int bs, nbx, nby; };

__global__ __launch_bounds__(kT) void slice_bwd_blocks_kernel(int N, Geo G, Img I, BlockShape S_, const float* __restrict__ rgb, int layout,
                                                              const int32_t* __restrict__ idx, int idx_stride, const float* __restrict__ grad_out,
                                                              int go_layout, float* __restrict__ slab, int4* __restrict__ table) {
    __shared__ float4 rec[4][kT];            // per staged pixel: {cell bits, fx, fy, fz}, dA[0..3], dA[4..7], dA[8..11]
    __shared__ float part[kT][13];           // the subsets' window sums
    __shared__ int red[4][kT / 64];
    const int t = threadIdx.x;
    const int b = blockIdx.y;
    const int blk = blockIdx.x;
    const int64_t row = (int64_t)b * gridDim.x + blk;
    const int64_t P = (int64_t)I.H * I.W;
    const int px0 = (blk % S_.nbx) * S_.bs, py0 = (blk / S_.nbx) * S_.bs;
    const int pw = min(S_.bs, I.W - px0), ph = min(S_.bs, I.H - py0);
    const int npx = pw * ph;
    const int g = grid_of(idx, idx_stride, b, N);
    if (g < 0) {                             // uniform over the workgroup
        if (t == 0) table[row] = make_int4(-1, 0, 0, 0);
        return;
    }
    const float* xyb = I.xy + b * I.xy_bstride;
    // the window: min / max of the floor cells, one vertex more on the high side (clamped)
    int mnx = 1 << 30, mny = 1 << 30, mxx = -1, mxy = -1;
    for (int q = t; q < npx; q += kT) {
        const int64_t p = (int64_t)(py0 + q / pw) * I.W + px0 + q % pw;
        int cx, cy;
        uv_cell(xyb[p * 2], xyb[p * 2 + 1], G, cx, cy);
        mnx = min(mnx, cx); mxx = max(mxx, cx);
        mny = min(mny, cy); mxy = max(mxy, cy);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mnx = min(mnx, __shfl_xor(mnx, off)); mxx = max(mxx, __shfl_xor(mxx, off));
        mny = min(mny, __shfl_xor(mny, off)); mxy = max(mxy, __shfl_xor(mxy, off));
    }
    if ((t & 63) == 0) { red[0][t >> 6] = mnx; red[1][t >> 6] = mxx; red[2][t >> 6] = mny; red[3][t >> 6] = mxy; }
    __syncthreads();
    mnx = red[0][0]; mxx = red[1][0]; mny = red[2][0]; mxy = red[3][0];
#pragma unroll
    for (int w = 1; w < kT / 64; ++w) {
        mnx = min(mnx, red[0][w]); mxx = max(mxx, red[1][w]);
        mny = min(mny, red[2][w]); mxy = max(mxy, red[3][w]);
    }
    const int vx0 = mnx, vx1 = min(mxx + 1, G.GW - 1), vy0 = mny, vy1 = min(mxy + 1, G.GH - 1);
    if (t == 0) table[row] = make_int4(g, vx0 | (vx1 << 16), vy0 | (vy1 << 16), 0);

    const int O = 9 * G.L, nsub = kT / O;
    const int o = t % O, s = t / O;
    const bool owner = s < nsub;
    const int jv = o / G.L, iz = o % G.L;
    float* srow = slab + row * 12 * G.LHW;
    for (int ty0 = vy0; ty0 <= vy1; ty0 += 3) {
        for (int tx0 = vx0; tx0 <= vx1; tx0 += 3) {
            const int vx = tx0 + jv % 3, vy = ty0 + jv / 3;
            float acc[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) acc[k] = 0.f;
            for (int c0 = 0; c0 < npx; c0 += kT) {
                __syncthreads();
                const int q = c0 + t;
                if (q < npx) {
                    const int64_t p = (int64_t)(py0 + q / pw) * I.W + px0 + q % pw;
                    const float cr = rgb[at(layout, b, P, p, 0)], cg = rgb[at(layout, b, P, p, 1)], cb = rgb[at(layout, b, P, p, 2)];
                    const Coords c = coords(xyb[p * 2], xyb[p * 2 + 1], cr, cg, cb, G);
                    const bool hit = c.x0 + 1 >= tx0 && c.x0 <= tx0 + 2 && c.y0 + 1 >= ty0 && c.y0 <= ty0 + 2;
                    const int cell = hit ? (c.x0 | (c.y0 << 10) | (c.z0 << 20)) : -1;
                    rec[0][t] = make_float4(__int_as_float(cell), c.fx, c.fy, c.fz);
                    float dA[12];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const float d = grad_out[at(go_layout, b, P, p, i)];
                        dA[4 * i] = d * cr; dA[4 * i + 1] = d * cg; dA[4 * i + 2] = d * cb; dA[4 * i + 3] = d;
                    }
                    rec[1][t] = make_float4(dA[0], dA[1], dA[2], dA[3]);
                    rec[2][t] = make_float4(dA[4], dA[5], dA[6], dA[7]);
                    rec[3][t] = make_float4(dA[8], dA[9], dA[10], dA[11]);
                }
                __syncthreads();
                if (owner) {
                    const int n = min(kT, npx - c0);
                    float ca[12];                    // this chunk's sum first: two-level, shorter rounding chains
#pragma unroll
                    for (int k = 0; k < 12; ++k) ca[k] = 0.f;
                    for (int j = s; j < n; j += nsub) {
                        const float4 h = rec[0][j];
                        const int cell = __float_as_int(h.x);
                        const int dx = vx - (cell & 1023), dy = vy - ((cell >> 10) & 1023), dz = iz - (cell >> 20);
                        const bool in = cell >= 0 && (unsigned)dx <= 1u && (unsigned)dy <= 1u && (unsigned)dz <= 1u;
                        const float wt = in ? (dx ? h.y : 1.f - h.y) * (dy ? h.z : 1.f - h.z) * (dz ? h.w : 1.f - h.w) : 0.f;
                        const float4 a = rec[1][j], bq = rec[2][j], cq = rec[3][j];
                        ca[0] += wt * a.x; ca[1] += wt * a.y; ca[2] += wt * a.z; ca[3] += wt * a.w;
                        ca[4] += wt * bq.x; ca[5] += wt * bq.y; ca[6] += wt * bq.z; ca[7] += wt * bq.w;
                        ca[8] += wt * cq.x; ca[9] += wt * cq.y; ca[10] += wt * cq.z; ca[11] += wt * cq.w;
                    }
#pragma unroll
                    for (int k = 0; k < 12; ++k) acc[k] += ca[k];
                }
            }
            // the subsets' sums, added in subset order by the owners of subset 0
            __syncthreads();
            if (owner) {
#pragma unroll
                for (int k = 0; k < 12; ++k) part[t][k] = acc[k];
            }
            __syncthreads();
            if (owner && s == 0 && vx <= vx1 && vy <= vy1) {
                for (int k = 0; k < 12; ++k) {
                    float v = part[o][k];
                    for (int u = 1; u < nsub; ++u) v += part[u * O + o][k];
                    srow[(int64_t)k * G.LHW + ((int64_t)iz * G.GH + vy) * G.GW + vx] = v;
                }
            }
        }
    }
}

// ---- slice backward: grid gradient, pass 2 (one thread per element of the dense gradient) ----------------------------------------
__global__ __launch_bounds__(kT) void slice_bwd_sum_kernel(Geo G, int B, int n_rows, const int32_t* __restrict__ idx, int idx_stride,
                                                           const float* __restrict__ slab, const int4* __restrict__ table,
                                                           float* __restrict__ grad_grids) {
    __shared__ int4 ent[kT];
    const int g = blockIdx.y;
    const int64_t E = 12 * G.LHW;
    const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
    bool used = false;
    for (int b = 0; b < B && !used; ++b) used = idx[(int64_t)b * idx_stride] == g;
    if (!used) {                                           // uniform: the whole workgroup writes zeros
        if (e < E) grad_grids[(int64_t)g * E + e] = 0.f;
        return;
    }
    const int ix = (int)(e % G.GW), iy = (int)((e / G.GW) % G.GH);
    float acc = 0.f;
    for (int r0 = 0; r0 < n_rows; r0 += kT) {
        __syncthreads();
        if (r0 + (int)threadIdx.x < n_rows) ent[threadIdx.x] = table[r0 + threadIdx.x];
        __syncthreads();
        const int n = min(kT, n_rows - r0);
        for (int j = 0; j < n; ++j) {
            const int4 h = ent[j];
            if (h.x != g) continue;
            if (ix < (h.y & 0xffff) || ix > (h.y >> 16) || iy < (h.z & 0xffff) || iy > (h.z >> 16)) continue;
            if (e < E) acc += slab[(int64_t)(r0 + j) * E + e];
        }
    }
    if (e < E) grad_grids[(int64_t)g * E + e] = acc;
}

// ---- total variation -----------------------------------------------------------------------------------------------------------------
struct Tv {
    int64_t n;                          // N C L GH GW
    int L, GH, GW;
    float inv_k[3];                     // 1 / K_d for d = L, GH, GW (0 where that size is 1)
};

__device__ inline float tv_elem(const float* __restrict__ x, int64_t i, const Tv& T) {
    const int ix = (int)(i % T.GW), iy = (int)((i / T.GW) % T.GH), iz = (int)((i / ((int64_t)T.GW * T.GH)) % T.L);
    const float v = x[i];
    float s = 0.f;
    if (ix + 1 < T.GW) { const float d = x[i + 1] - v; s += d * d * T.inv_k[2]; }
    if (iy + 1 < T.GH) { const float d = x[i + T.GW] - v; s += d * d * T.inv_k[1]; }
    if (iz + 1 < T.L) { const float d = x[i + (int64_t)T.GW * T.GH] - v; s += d * d * T.inv_k[0]; }
    return s;
}

// (the sums: block_sum of gspl_reduce.h, lanes by xor butterfly, then the four waves in order)
__global__ __launch_bounds__(kT) void tv_partials_kernel(Tv T, const float* __restrict__ x, float* __restrict__ partials) {
    __shared__ float sh[kT / 64];
    float a = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < T.n; i += (int64_t)gridDim.x * kT) a += tv_elem(x, i, T);
    const float s = block_sum<kT>(a, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(kT) void tv_final_kernel(int n_partials, float inv_n, const float* __restrict__ partials, float* __restrict__ out) {
    __shared__ float sh[kT / 64];
    float a = 0.f;
    for (int j = threadIdx.x; j < n_partials; j += kT) a += partials[j];
    const float s = block_sum<kT>(a, sh);
    if (threadIdx.x == 0) out[0] = s * inv_n;
}

__global__ __launch_bounds__(kT) void tv_bwd_kernel(Tv T, float inv_n, const float* __restrict__ x, const float* __restrict__ grad_out,
                                                    float* __restrict__ grad_x) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= T.n) return;
    const int ix = (int)(i % T.GW), iy = (int)((i / T.GW) % T.GH), iz = (int)((i / ((int64_t)T.GW * T.GH)) % T.L);
    const int64_t zs = (int64_t)T.GW * T.GH;
    const float v = x[i];
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (ix > 0) gx += v - x[i - 1];
    if (ix + 1 < T.GW) gx -= x[i + 1] - v;
    if (iy > 0) gy += v - x[i - T.GW];
    if (iy + 1 < T.GH) gy -= x[i + T.GW] - v;
    if (iz > 0) gz += v - x[i - zs];
    if (iz + 1 < T.L) gz -= x[i + zs] - v;
    const float s = 2.f * grad_out[0] * inv_n;
    grad_x[i] = s * (gx * T.inv_k[2] + gy * T.inv_k[1] + gz * T.inv_k[0]);
}

inline bool grid_ok(int N, int L, int GH, int GW) {
    return N >= 1 && N <= 65535 && L >= 1 && GH >= 1 && GW >= 1 && L <= kMaxL && GH <= kMaxXY && GW <= kMaxXY &&
           (int64_t)L * GH * GW <= kMaxVertices;
}

// the smallest block side (64 << k) with at most 512 blocks and 64 MiB of slab per image (or a single block)
inline BlockShape block_shape(int L, int GH, int GW, int H, int W) {
    const size_t row_bytes = (size_t)12 * L * GH * GW * sizeof(float);
    BlockShape s;
    for (int bs = kMinBlock;; bs *= 2) {
        s.bs = bs;
        s.nbx = (W + bs - 1) / bs;
        s.nby = (H + bs - 1) / bs;
        const int64_t n = (int64_t)s.nbx * s.nby;
        if (n == 1 || (n <= kMaxBlocksPerImage && (size_t)n * row_bytes <= kSlabBytesPerImage)) return s;
    }
}

inline Tv tv_shape(int N, int C, int L, int GH, int GW) {
    Tv T;
    T.n = (int64_t)N * C * L * GH * GW;
    T.L = L; T.GH = GH; T.GW = GW;
    const int sz[3] = {L, GH, GW};
    for (int d = 0; d < 3; ++d) {
        double k = (double)C * (sz[d] - 1);
        for (int e = 0; e < 3; ++e)
            if (e != d) k *= sz[e];
        T.inv_k[d] = sz[d] > 1 ? (float)(1.0 / k) : 0.f;
    }
    return T;
}

}  // namespace
}  // namespace gspl

extern "C" size_t gspl_bilagrid_workspace_bytes(int L, int GH, int GW, int B, int H, int W) {
    using namespace gspl;
    if (!grid_ok(1, L, GH, GW) || B < 1 || H < 1 || W < 1) return 0;
    const BlockShape s = block_shape(L, GH, GW, H, W);
    const size_t rows = (size_t)B * s.nbx * s.nby;
    return rows * sizeof(int4) + rows * (size_t)12 * L * GH * GW * sizeof(float);   // the block table, then the slab rows
}

extern "C" int gspl_bilagrid_slice_fwd(int N, int L, int GH, int GW, int B, int H, int W, const float* grids, const float* xy,
                                       int64_t xy_bstride, const float* rgb, int layout, const int32_t* idx, int idx_stride, float* out,
                                       void* stream) {
    using namespace gspl;
    if (!grid_ok(N, L, GH, GW))
        return fail_arg("bilagrid_slice_fwd: grid size out of bounds (1 <= N <= 65535, L <= 28, GH, GW <= 1024, L GH GW <= 16384)");
    if (B < 1 || B > 65535 || H < 0 || W < 0 || (layout != GSPL_LAYOUT_HWC && layout != GSPL_LAYOUT_CHW))
        return fail_arg("bilagrid_slice_fwd: bad image shape or layout");
    if ((int64_t)H * W == 0) return GSPL_OK;
    if (!grids || !xy || !rgb || !idx || !out) return fail_arg("bilagrid_slice_fwd: NULL pointer");
    const Geo G{L, GH, GW, (int64_t)L * GH * GW};
    const Img I{B, H, W, xy, xy_bstride};
    const dim3 grid((unsigned)(((int64_t)H * W + kT - 1) / kT), (unsigned)B);
    hipLaunchKernelGGL(slice_fwd_kernel, grid, dim3(kT), 0, (hipStream_t)stream, N, G, I, grids, rgb, layout, idx, idx_stride, out);
    return check_launch("bilagrid_slice_fwd");
}

extern "C" int gspl_bilagrid_slice_bwd(int N, int L, int GH, int GW, int B, int H, int W, const float* grids, const float* xy,
                                       int64_t xy_bstride, const float* rgb, int layout, const int32_t* idx, int idx_stride,
                                       const float* grad_out, int go_layout, float* grad_grids, float* grad_rgb, int gr_layout,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    using namespace gspl;
    if (!grid_ok(N, L, GH, GW))
        return fail_arg("bilagrid_slice_bwd: grid size out of bounds (1 <= N <= 65535, L <= 28, GH, GW <= 1024, L GH GW <= 16384)");
    const bool lay_ok = (layout == GSPL_LAYOUT_HWC || layout == GSPL_LAYOUT_CHW) && (go_layout == GSPL_LAYOUT_HWC || go_layout == GSPL_LAYOUT_CHW) &&
                        (gr_layout == GSPL_LAYOUT_HWC || gr_layout == GSPL_LAYOUT_CHW);
    if (B < 1 || B > 65535 || H < 0 || W < 0 || !lay_ok) return fail_arg("bilagrid_slice_bwd: bad image shape or layout");
    if (!grids || !xy || !rgb || !idx || !grad_out) return fail_arg("bilagrid_slice_bwd: NULL pointer");
    const Geo G{L, GH, GW, (int64_t)L * GH * GW};
    const Img I{B, H, W, xy, xy_bstride};
    const hipStream_t s = (hipStream_t)stream;
    const int64_t P = (int64_t)H * W;
    if (grad_rgb && P > 0) {
        const dim3 grid((unsigned)((P + kT - 1) / kT), (unsigned)B);
        hipLaunchKernelGGL(slice_bwd_rgb_kernel, grid, dim3(kT), 0, s, N, G, I, grids, rgb, layout, idx, idx_stride, grad_out, go_layout,
                           grad_rgb, gr_layout);
        const int rc = check_launch("bilagrid_slice_bwd (colour)");
        if (rc != GSPL_OK) return rc;
    }
    if (!grad_grids) return GSPL_OK;
    int rows = 0;
    int4* table = nullptr;
    float* slab = nullptr;
    if (P > 0) {
        const BlockShape bsh = block_shape(L, GH, GW, H, W);
        rows = B * bsh.nbx * bsh.nby;
        if (!workspace || workspace_bytes < gspl_bilagrid_workspace_bytes(L, GH, GW, B, H, W) || (reinterpret_cast<uintptr_t>(workspace) & 15u))
            return fail_ws("bilagrid_slice_bwd: workspace (gspl_bilagrid_workspace_bytes, 16-byte aligned)");
        table = static_cast<int4*>(workspace);
        slab = reinterpret_cast<float*>(table + rows);
        hipLaunchKernelGGL(slice_bwd_blocks_kernel, dim3((unsigned)(bsh.nbx * bsh.nby), (unsigned)B), dim3(kT), 0, s, N, G, I, bsh, rgb, layout,
                           idx, idx_stride, grad_out, go_layout, slab, table);
        const int rc = check_launch("bilagrid_slice_bwd (blocks)");
        if (rc != GSPL_OK) return rc;
    }
    const int64_t E = 12 * G.LHW;
    hipLaunchKernelGGL(slice_bwd_sum_kernel, dim3((unsigned)((E + kT - 1) / kT), (unsigned)N), dim3(kT), 0, s, G, P > 0 ? B : 0, rows, idx,
                       idx_stride, slab, table, grad_grids);
    return check_launch("bilagrid_slice_bwd (sum)");
}

extern "C" int gspl_bilagrid_tv_partials(int64_t n) {
    using namespace gspl;
    if (n <= 0) return 1;
    const int64_t g = (n + kTvPerPartial - 1) / kTvPerPartial;
    return (int)(g < kTvMaxPartials ? g : kTvMaxPartials);
}

extern "C" int gspl_bilagrid_tv_fwd(int N, int C, int L, int GH, int GW, const float* x, float* partials, float* out, void* stream) {
    using namespace gspl;
    if (N < 1 || C < 1 || L < 1 || GH < 1 || GW < 1) return fail_arg("bilagrid_tv_fwd: every size must be positive");
    if (!x || !partials || !out) return fail_arg("bilagrid_tv_fwd: NULL pointer");
    const Tv T = tv_shape(N, C, L, GH, GW);
    const int np = gspl_bilagrid_tv_partials(T.n);
    hipLaunchKernelGGL(tv_partials_kernel, dim3(np), dim3(kT), 0, (hipStream_t)stream, T, x, partials);
    const int rc = check_launch("bilagrid_tv_fwd");
    if (rc != GSPL_OK) return rc;
    hipLaunchKernelGGL(tv_final_kernel, dim3(1), dim3(kT), 0, (hipStream_t)stream, np, 1.f / (float)N, partials, out);
    return check_launch("bilagrid_tv_fwd");
}

extern "C" int gspl_bilagrid_tv_bwd(int N, int C, int L, int GH, int GW, const float* x, const float* grad_out, float* grad_x, void* stream) {
    using namespace gspl;
    if (N < 1 || C < 1 || L < 1 || GH < 1 || GW < 1) return fail_arg("bilagrid_tv_bwd: every size must be positive");
    if (!x || !grad_out || !grad_x) return fail_arg("bilagrid_tv_bwd: NULL pointer");
    const Tv T = tv_shape(N, C, L, GH, GW);
    hipLaunchKernelGGL(tv_bwd_kernel, dim3((unsigned)((T.n + kT - 1) / kT)), dim3(kT), 0, (hipStream_t)stream, T, 1.f / (float)N, x, grad_out, grad_x);
    return check_launch("bilagrid_tv_bwd");
}

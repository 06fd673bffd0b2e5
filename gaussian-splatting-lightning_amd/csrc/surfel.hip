// surfel.hip — the 2D Gaussian Splatting (surfel) rasterizer: preprocess, compositing, their backward, and the one C-ABI call per
// direction (`gspl_rasterize_surfel_fwd/bwd`, include/gspl_hip.h section 6c).
//
// Replaces `diff_surfel_rasterization.GaussianRasterizer` (reference call site internal/renderers/vanilla_2dgs_renderer.py:50-90).
// The package is not vendored in the reference; the algorithm restated here is the published 2DGS rasterizer (hbb1), in the
// conventions of the Inria path of this library (row-vector viewmatrix / projmatrix, pixel centres at integer coordinates):
//   per splat   cull view z <= 0.2; t_u = R[:,0] s_u mod, t_v = R[:,1] s_v mod (R: the normalised quaternion), world normal R[:,2];
//               M = S2W P N (3x3), S2W rows [t_u,0] [t_v,0] [p,1], N the NDC -> pixel map; Tu / Tv / Tw = the x / y / w columns of M;
//               t = (9, 9, -1), d = t.(Tw Tw), cull d == 0, f = t / d, centre = (f.(Tu Tw), f.(Tv Tw)),
//               h = sqrt(max(1e-4, centre^2 - (f.(Tu Tu), f.(Tv Tv)))) (evaluated without cancellation), radius = ceil(max(h.x, h.y, 3 FilterSize)), Inria tile rect;
//               view normal flipped towards the camera (cull cos == 0); colour from SH (+0.5, clamp) or colors_precomp.
//   per pixel   k = x Tw - Tu, l = y Tw - Tv, p = k x l (skip p.z == 0), s = p.xy / p.z, rho3 = |s|^2, rho2 = |centre - x|^2 / FilterSize^2,
//               z = rho3 <= rho2 ? s.Tw.xy + Tw.z : Tw.z (skip z < 0.2), alpha = min(0.99, o exp(-min(rho3, rho2) / 2)) (skip < 1/255,
//               stop when T (1 - alpha) < 1e-4), w = alpha T: colour, depth, normal, alpha, median depth (T > 0.5 before the update),
//               distortion sum_i sum_j<i w_i w_j (m_i - m_j)^2 with m = far / (far - near) (1 - near / z).
// Backward: the exact derivative with the 0.99 clamp straight-through, no gradient through a clamped SH channel, and upstream's
// densification proxy in means2D (see gspl_hip.h 6c).  Parity with the CUDA package is unpinned: tests/surfel_oracle.py pins this
// restatement in fp64.
//
// Binning is the library's list-only binning (gspl_bin_count / gspl_bin_emit_sort) without the conic tile culling, on the centres
// and radii above.  Compositing: one 16x16 tile per workgroup, the per-splat record (Tu Tv Tw | centre | opacity | normal | rgb,
// 18 floats) staged in LDS.  The backward walks each tile back to front, reduces the 18 gradient values of a (tile, splat) over the
// wave with DPP and over the four waves in LDS, then issues one float atomic per value into a contiguous [N, 18] row
// (gspl_get_deterministic(): one row per list entry instead, added up per splat in list order).
// Floating-point contraction as the language defines it: the forward and the backward kernels evaluate the per-pixel intersection
// through one function and must take the same skip / stop decisions.
#pragma clang fp contract(on)
#include "gspl_composite.h"
#include <cstring>

namespace gspl {

static constexpr float SURF_C = 3.f;                         // cutoff in sigma
static constexpr float SURF_FILTER = 0.707106f;              // FilterSize
static constexpr float SURF_FILTER_INV_SQ = 1.f / (0.707106f * 0.707106f);
static constexpr float SURF_NEAR = 0.2f, SURF_FAR = 100.f;
static constexpr int SURF_REC = 16;                          // floats per record in HBM: Tu Tv Tw | cx cy | opacity | n | 0 (one 64-B line)
static constexpr int SURF_GRAD = 18;                         // floats per gradient row: Tu Tv Tw | cx cy | opacity | n | rgb
static constexpr int SURF_LDS = 18;                          // floats per staged record: the 16 above without the pad, then rgb

// ---- per-splat geometry (preprocess forward and backward) ----------------------------------------------------------------------
struct SurfelGeom {
    float pv[3];
    float qn[4], qlen;
    float R[9];
    float su, sv;              // scales times the modifier
    float a[3][3], b[3];       // Q = P N: column j is (a[j][0..2], b[j]) (rows 0..2 of P N, then row 3)
    float Tu[3], Tv[3], Tw[3];
    float f[3], cx, cy;
    float n[3];                // view-space normal, flipped towards the camera
    float sign;                // +1 / -1: the flip
};

// false: culled
__device__ __forceinline__ bool surfel_geom(const float* __restrict__ V, const float* __restrict__ P, const float p[3], const float q_in[4],
                                            const float s_in[2], float mod, int W, int H, SurfelGeom& G) {
#pragma unroll
    for (int c = 0; c < 3; ++c) G.pv[c] = p[0] * V[0 * 4 + c] + p[1] * V[1 * 4 + c] + p[2] * V[2 * 4 + c] + V[12 + c];
    if (G.pv[2] <= SURF_NEAR) return false;
    G.qlen = sqrtf(q_in[0] * q_in[0] + q_in[1] * q_in[1] + q_in[2] * q_in[2] + q_in[3] * q_in[3]);
    const float iq = 1.f / G.qlen;
#pragma unroll
    for (int j = 0; j < 4; ++j) G.qn[j] = q_in[j] * iq;
    quat_to_rotmat(G.qn, G.R);
    G.su = s_in[0] * mod; G.sv = s_in[1] * mod;
    const float tu[3] = {G.R[0] * G.su, G.R[3] * G.su, G.R[6] * G.su};
    const float tv[3] = {G.R[1] * G.sv, G.R[4] * G.sv, G.R[7] * G.sv};
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H, ow = 0.5f * (float)(W - 1), oh = 0.5f * (float)(H - 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float c0 = P[i * 4 + 0] * hw + P[i * 4 + 3] * ow;
        const float c1 = P[i * 4 + 1] * hh + P[i * 4 + 3] * oh;
        const float c2 = P[i * 4 + 3];
        if (i < 3) { G.a[0][i] = c0; G.a[1][i] = c1; G.a[2][i] = c2; }
        else { G.b[0] = c0; G.b[1] = c1; G.b[2] = c2; }
    }
    float* T[3] = {G.Tu, G.Tv, G.Tw};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        T[j][0] = tu[0] * G.a[j][0] + tu[1] * G.a[j][1] + tu[2] * G.a[j][2];
        T[j][1] = tv[0] * G.a[j][0] + tv[1] * G.a[j][1] + tv[2] * G.a[j][2];
        T[j][2] = p[0] * G.a[j][0] + p[1] * G.a[j][1] + p[2] * G.a[j][2] + G.b[j];
    }
    const float c2 = SURF_C * SURF_C;
    const float d = c2 * G.Tw[0] * G.Tw[0] + c2 * G.Tw[1] * G.Tw[1] - G.Tw[2] * G.Tw[2];
    if (d == 0.f) return false;
    G.f[0] = c2 / d; G.f[1] = c2 / d; G.f[2] = -1.f / d;
    G.cx = G.f[0] * G.Tu[0] * G.Tw[0] + G.f[1] * G.Tu[1] * G.Tw[1] + G.f[2] * G.Tu[2] * G.Tw[2];
    G.cy = G.f[0] * G.Tv[0] * G.Tw[0] + G.f[1] * G.Tv[1] * G.Tw[1] + G.f[2] * G.Tv[2] * G.Tw[2];
    const float nw[3] = {G.R[2], G.R[5], G.R[8]};
#pragma unroll
    for (int c = 0; c < 3; ++c) G.n[c] = nw[0] * V[0 * 4 + c] + nw[1] * V[1 * 4 + c] + nw[2] * V[2 * 4 + c];
    const float cosv = -(G.pv[0] * G.n[0] + G.pv[1] * G.n[1] + G.pv[2] * G.n[2]);
    if (cosv == 0.f) return false;
    G.sign = cosv < 0.f ? -1.f : 1.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) G.n[c] *= G.sign;
    return true;
}

// colors_precomp (nullable): copied into `colors` for the rows that are not culled
__global__ __launch_bounds__(256) void surfel_preprocess_fwd_kernel(
    int N, const float* __restrict__ means, const float* __restrict__ scales, const float* __restrict__ quats,
    const float* __restrict__ opacities, const float* __restrict__ viewmatrix, const float* __restrict__ projmatrix,
    int W, int H, float mod, const float* __restrict__ colors_precomp,
    int32_t* __restrict__ radii, float* __restrict__ means2d, float* __restrict__ depths, float* __restrict__ rec, float* __restrict__ colors) {
    __shared__ float s_cam[32];
    if (threadIdx.x < 16) { s_cam[threadIdx.x] = viewmatrix[threadIdx.x]; s_cam[16 + threadIdx.x] = projmatrix[threadIdx.x]; }
    __syncthreads();
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= N) return;
    const float p[3] = {means[g * 3 + 0], means[g * 3 + 1], means[g * 3 + 2]};
    const float q[4] = {quats[g * 4 + 0], quats[g * 4 + 1], quats[g * 4 + 2], quats[g * 4 + 3]};
    const float s[2] = {scales[g * 2 + 0], scales[g * 2 + 1]};
    SurfelGeom G;
    int radius = 0;
    if (surfel_geom(s_cam, s_cam + 16, p, q, s, mod, W, H, G)) {
        // centre^2 - f.(Tu Tu) without its cancellation (centre ~ 1e3 px, the difference ~ h^2): with D = diag(9, 9, -1),
        // (u.D w)^2 - (u.D u)(w.D w) = -sum_{i<j} D_i D_j (u_i w_j - u_j w_i)^2, so the extent is (9 (m02^2 + m12^2) - 81 m01^2) / d^2
        const float inv_d2 = G.f[2] * G.f[2];
        auto extent2 = [&](const float* u) {
            const float m01 = u[0] * G.Tw[1] - u[1] * G.Tw[0], m02 = u[0] * G.Tw[2] - u[2] * G.Tw[0], m12 = u[1] * G.Tw[2] - u[2] * G.Tw[1];
            return (9.f * (m02 * m02 + m12 * m12) - 81.f * (m01 * m01)) * inv_d2;
        };
        const float ex = extent2(G.Tu), ey = extent2(G.Tv);
        const float hx = sqrtf(fmaxf(1e-4f, ex)), hy = sqrtf(fmaxf(1e-4f, ey));
        const int r = (int)ceilf(fmaxf(fmaxf(hx, hy), SURF_C * SURF_FILTER));
        const int grid_x = (W + 15) / 16, grid_y = (H + 15) / 16;
        const float rf = (float)r;
        const int minx = min(grid_x, max(0, (int)((G.cx - rf) / 16.f)));
        const int miny = min(grid_y, max(0, (int)((G.cy - rf) / 16.f)));
        const int maxx = min(grid_x, max(0, (int)((G.cx + rf + 15.f) / 16.f)));
        const int maxy = min(grid_y, max(0, (int)((G.cy + rf + 15.f) / 16.f)));
        if ((maxx - minx) * (maxy - miny) > 0) radius = r;
    }
    float4* out = reinterpret_cast<float4*>(rec + (int64_t)g * SURF_REC);
    radii[g] = radius;
    if (radius > 0) {
        means2d[g * 2 + 0] = G.cx; means2d[g * 2 + 1] = G.cy;
        depths[g] = G.pv[2];
        out[0] = make_float4(G.Tu[0], G.Tu[1], G.Tu[2], G.Tv[0]);
        out[1] = make_float4(G.Tv[1], G.Tv[2], G.Tw[0], G.Tw[1]);
        out[2] = make_float4(G.Tw[2], G.cx, G.cy, opacities[g]);
        out[3] = make_float4(G.n[0], G.n[1], G.n[2], 0.f);
    } else {
        means2d[g * 2 + 0] = 0.f; means2d[g * 2 + 1] = 0.f;
        depths[g] = 0.f;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        out[0] = z; out[1] = z; out[2] = z; out[3] = z;
    }
    if (colors_precomp) {
#pragma unroll
        for (int c = 0; c < 3; ++c) colors[g * 3 + c] = radius > 0 ? colors_precomp[g * 3 + c] : 0.f;
    }
}

// ---- per-pixel intersection, shared by the two compositing kernels ---------------------------------------------------------
struct SurfelHit {
    float k[3], l[3], p[3];
    float s0, s1, ipz;
    float dx, dy;
    float z, G, alpha;
    bool use3;
};
// r: the staged record (LDS); false: the splat is skipped at this pixel (p.z == 0, z < near, alpha < 1/255)
__device__ __forceinline__ bool surfel_hit(const float* r, float x, float y, SurfelHit& h) {
    const float Tu0 = r[0], Tu1 = r[1], Tu2 = r[2], Tv0 = r[3], Tv1 = r[4], Tv2 = r[5], Tw0 = r[6], Tw1 = r[7], Tw2 = r[8];
    h.k[0] = x * Tw0 - Tu0; h.k[1] = x * Tw1 - Tu1; h.k[2] = x * Tw2 - Tu2;
    h.l[0] = y * Tw0 - Tv0; h.l[1] = y * Tw1 - Tv1; h.l[2] = y * Tw2 - Tv2;
    h.p[0] = h.k[1] * h.l[2] - h.k[2] * h.l[1];
    h.p[1] = h.k[2] * h.l[0] - h.k[0] * h.l[2];
    h.p[2] = h.k[0] * h.l[1] - h.k[1] * h.l[0];
    if (h.p[2] == 0.f) return false;
    h.ipz = 1.f / h.p[2];
    h.s0 = h.p[0] * h.ipz; h.s1 = h.p[1] * h.ipz;
    const float rho3 = h.s0 * h.s0 + h.s1 * h.s1;
    h.dx = r[9] - x; h.dy = r[10] - y;
    const float rho2 = SURF_FILTER_INV_SQ * (h.dx * h.dx + h.dy * h.dy);
    h.use3 = rho3 <= rho2;
    h.z = h.use3 ? h.s0 * Tw0 + h.s1 * Tw1 + Tw2 : Tw2;
    if (h.z < SURF_NEAR) return false;
    h.G = __expf(-0.5f * fminf(rho3, rho2));
    h.alpha = fminf(0.99f, r[11] * h.G);
    return h.alpha >= kAlphaMin;
}

__device__ __forceinline__ void surfel_range(int tile, int n_tiles, int64_t n_isects, const int32_t* __restrict__ offsets, int& start, int& end) {
    if (n_isects <= 0) { start = end = 0; return; }      // (no list: `offsets` is not read)
    tile_range(tile, n_tiles, n_isects, offsets, start, end);
}

// stage the record of list entry `idx` into s (18 floats)
__device__ __forceinline__ void surfel_stage(const float* __restrict__ rec, const float* __restrict__ colors, int id, float* s) {
    const float4* r4 = reinterpret_cast<const float4*>(rec + (int64_t)id * SURF_REC);
    const float4 a = r4[0], b = r4[1], c = r4[2], d = r4[3];
    s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w;
    s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
    s[8] = c.x; s[9] = c.y; s[10] = c.z; s[11] = c.w;
    s[12] = d.x; s[13] = d.y; s[14] = d.z;
    s[15] = colors[id * 3 + 0]; s[16] = colors[id * 3 + 1]; s[17] = colors[id * 3 + 2];
}

static constexpr float SURF_M_SCALE = SURF_FAR / (SURF_FAR - SURF_NEAR);

// out_color [3,H,W] (+ T bg), out_all [7,H,W]: depth | alpha | normal (3) | median depth | distortion.
// Per pixel for the backward: final T, M1, M2, one past the last contributor's list index (the tile's start: none), the median
// contributor's list index (-1: none).
__global__ __launch_bounds__(256) void surfel_fwd_kernel(
    int W, int H, int tile_w, int n_tiles, int64_t n_isects, const int32_t* __restrict__ offsets, const int32_t* __restrict__ flat,
    const float* __restrict__ rec, const float* __restrict__ colors, const float* __restrict__ bg,
    float* __restrict__ out_color, float* __restrict__ out_all, float* __restrict__ final_T, float* __restrict__ out_M1, float* __restrict__ out_M2,
    int32_t* __restrict__ last_contrib, int32_t* __restrict__ median_contrib) {
    __shared__ float s_rec[256 * SURF_LDS];
    const int tile = blockIdx.x;
    const int px = (tile % tile_w) * 16 + (threadIdx.x & 15), py = (tile / tile_w) * 16 + (threadIdx.x >> 4);
    const bool inside = px < W && py < H;
    const float x = (float)px, y = (float)py;
    int start, end;
    surfel_range(tile, n_tiles, n_isects, offsets, start, end);
    float T = 1.f, C0 = 0.f, C1 = 0.f, C2 = 0.f, D = 0.f, N0 = 0.f, N1 = 0.f, N2 = 0.f, M1 = 0.f, M2 = 0.f, dist = 0.f, med = 0.f;
    int last = start, med_idx = -1;
    bool done = !inside;
    for (int b0 = start; b0 < end; b0 += 256) {
        if (__syncthreads_count(done) == 256) break;
        const int i = b0 + (int)threadIdx.x;
        if (i < end) surfel_stage(rec, colors, flat[i], s_rec + threadIdx.x * SURF_LDS);
        __syncthreads();
        const int n = min(256, end - b0);
        for (int j = 0; j < n && !done; ++j) {
            const float* r = s_rec + j * SURF_LDS;
            SurfelHit h;
            if (!surfel_hit(r, x, y, h)) continue;
            const float test_T = T * (1.f - h.alpha);
            if (test_T < kTStop) { done = true; break; }
            const float w = h.alpha * T;
            C0 += w * r[15]; C1 += w * r[16]; C2 += w * r[17];
            D += w * h.z;
            N0 += w * r[12]; N1 += w * r[13]; N2 += w * r[14];
            const float A = 1.f - T;
            const float m = SURF_M_SCALE * (1.f - SURF_NEAR / h.z);
            dist += w * (m * m * A + M2 - 2.f * m * M1);
            M1 += w * m;
            M2 += w * m * m;
            if (T > 0.5f) { med = h.z; med_idx = b0 + j; }
            T = test_T;
            last = b0 + j + 1;
        }
    }
    if (!inside) return;
    const int pix = py * W + px, HW = W * H;
    out_color[0 * HW + pix] = C0 + T * bg[0];
    out_color[1 * HW + pix] = C1 + T * bg[1];
    out_color[2 * HW + pix] = C2 + T * bg[2];
    out_all[0 * HW + pix] = D;
    out_all[1 * HW + pix] = 1.f - T;
    out_all[2 * HW + pix] = N0;
    out_all[3 * HW + pix] = N1;
    out_all[4 * HW + pix] = N2;
    out_all[5 * HW + pix] = med;
    out_all[6 * HW + pix] = dist;
    final_T[pix] = T; out_M1[pix] = M1; out_M2[pix] = M2;
    last_contrib[pix] = last; median_contrib[pix] = med_idx;
}

static constexpr int SURF_BB = 32;      // splats per backward batch

// v_rows [N,18] (atomics; zero-initialised) or, with `entries` != NULL, one row per list entry [n_isects,18] (single writer)
__global__ __launch_bounds__(256) void surfel_bwd_kernel(
    int W, int H, int tile_w, int n_tiles, int64_t n_isects, const int32_t* __restrict__ offsets, const int32_t* __restrict__ flat,
    const float* __restrict__ rec, const float* __restrict__ colors, const float* __restrict__ bg,
    const float* __restrict__ final_T, const float* __restrict__ fM1, const float* __restrict__ fM2,
    const int32_t* __restrict__ last_contrib, const int32_t* __restrict__ median_contrib,
    const float* __restrict__ v_color, const float* __restrict__ v_all, float* __restrict__ v_rows, float* __restrict__ entries) {
    __shared__ float s_rec[SURF_BB * SURF_LDS];
    __shared__ int s_id[SURF_BB];
    __shared__ float s_grad[4][SURF_BB][SURF_GRAD];
    __shared__ int s_any[4][SURF_BB];
    __shared__ int s_max;
    const int tile = blockIdx.x;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int px = (tile % tile_w) * 16 + (t & 15), py = (tile / tile_w) * 16 + (t >> 4);
    const bool inside = px < W && py < H;
    const float x = (float)px, y = (float)py;
    int start, end;
    surfel_range(tile, n_tiles, n_isects, offsets, start, end);
    if (start >= end) return;
    const int pix = py * W + px, HW = W * H;
    float Tc = 1.f, A_tot = 0.f, M1 = 0.f, M2 = 0.f;
    float gC0 = 0.f, gC1 = 0.f, gC2 = 0.f, gD = 0.f, gA = 0.f, gN0 = 0.f, gN1 = 0.f, gN2 = 0.f, gMed = 0.f, gDist = 0.f;
    int last = start, medi = -1;
    if (inside) {
        Tc = final_T[pix]; A_tot = 1.f - Tc; M1 = fM1[pix]; M2 = fM2[pix];
        last = last_contrib[pix]; medi = median_contrib[pix];
        gC0 = v_color[0 * HW + pix]; gC1 = v_color[1 * HW + pix]; gC2 = v_color[2 * HW + pix];
        gD = v_all[0 * HW + pix]; gA = v_all[1 * HW + pix];
        gN0 = v_all[2 * HW + pix]; gN1 = v_all[3 * HW + pix]; gN2 = v_all[4 * HW + pix];
        gMed = v_all[5 * HW + pix]; gDist = v_all[6 * HW + pix];
    }
    float acc = gC0 * bg[0] + gC1 * bg[1] + gC2 * bg[2];      // (sum_{j > i} w_j f_j + T_final f_bg) / T_{i+1}
    if (t == 0) s_max = start;
    __syncthreads();
    atomicMax(&s_max, last);
    __syncthreads();
    const int walk_end = s_max;
    for (int bend = walk_end; bend > start; bend -= SURF_BB) {
        const int n = min(SURF_BB, bend - start);
        if (t < n) {
            const int id = flat[bend - 1 - t];
            s_id[t] = id;
            surfel_stage(rec, colors, id, s_rec + t * SURF_LDS);
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const int idx = bend - 1 - j;
            const float* r = s_rec + j * SURF_LDS;
            float g[SURF_GRAD];
#pragma unroll
            for (int k = 0; k < SURF_GRAD; ++k) g[k] = 0.f;
            SurfelHit h;
            const bool contrib = inside && idx < last && surfel_hit(r, x, y, h);
            if (contrib) {
                const float Ti = Tc / (1.f - h.alpha);
                const float w = h.alpha * Ti;
                const float m = SURF_M_SCALE * (1.f - SURF_NEAR / h.z);
                const float e = m * m * A_tot - 2.f * m * M1 + M2;
                const float f = r[15] * gC0 + r[16] * gC1 + r[17] * gC2 + h.z * gD + r[12] * gN0 + r[13] * gN1 + r[14] * gN2 + gA + gDist * e;
                const float g_alpha = Ti * (f - acc);
                acc = h.alpha * f + (1.f - h.alpha) * acc;
                Tc = Ti;
                g[15] = w * gC0; g[16] = w * gC1; g[17] = w * gC2;
                g[12] = w * gN0; g[13] = w * gN1; g[14] = w * gN2;
                float gz = w * gD + 2.f * gDist * w * (m * A_tot - M1) * SURF_M_SCALE * SURF_NEAR / (h.z * h.z);
                if (idx == medi) gz += gMed;
                g[11] = g_alpha * h.G;                              // straight-through 0.99 clamp
                const float g_rho = -0.5f * g_alpha * r[11] * h.G;
                if (h.use3) {
                    const float gs0 = 2.f * g_rho * h.s0 + gz * r[6];
                    const float gs1 = 2.f * g_rho * h.s1 + gz * r[7];
                    g[6] += gz * h.s0; g[7] += gz * h.s1; g[8] += gz;
                    const float gp0 = gs0 * h.ipz, gp1 = gs1 * h.ipz, gp2 = -(gs0 * h.s0 + gs1 * h.s1) * h.ipz;
                    // p = k x l: dL/dk = l x gp, dL/dl = gp x k
                    const float gk0 = h.l[1] * gp2 - h.l[2] * gp1, gk1 = h.l[2] * gp0 - h.l[0] * gp2, gk2 = h.l[0] * gp1 - h.l[1] * gp0;
                    const float gl0 = gp1 * h.k[2] - gp2 * h.k[1], gl1 = gp2 * h.k[0] - gp0 * h.k[2], gl2 = gp0 * h.k[1] - gp1 * h.k[0];
                    g[0] = -gk0; g[1] = -gk1; g[2] = -gk2;
                    g[3] = -gl0; g[4] = -gl1; g[5] = -gl2;
                    g[6] += x * gk0 + y * gl0; g[7] += x * gk1 + y * gl1; g[8] += x * gk2 + y * gl2;
                } else {
                    g[9] = 2.f * SURF_FILTER_INV_SQ * g_rho * h.dx;
                    g[10] = 2.f * SURF_FILTER_INV_SQ * g_rho * h.dy;
                    g[8] += gz;
                }
            }
            // wave-uniform: a wave none of whose pixels composited this splat skips the reduction
            const unsigned long long any = __ballot(contrib);
            if (any) {
#pragma unroll
                for (int k = 0; k < SURF_GRAD; ++k) g[k] = wave_sum_to_lane63(g[k]);
                if (lane == 63) {
#pragma unroll
                    for (int k = 0; k < SURF_GRAD; ++k) s_grad[wave][j][k] = g[k];
                }
            }
            if (lane == 0) s_any[wave][j] = any != 0ull;
        }
        __syncthreads();
        // flush: the batch's rows, contiguous values of consecutive rows per instruction; rows nobody composited are skipped
        for (int e = t; e < n * SURF_GRAD; e += 256) {
            const int j = e / SURF_GRAD, k = e - j * SURF_GRAD;
            float v = 0.f;
            bool used = false;
#pragma unroll
            for (int w4 = 0; w4 < 4; ++w4) if (s_any[w4][j]) { v += s_grad[w4][j][k]; used = true; }
            if (!used) continue;
            if (entries) entries[(int64_t)(bend - 1 - j) * SURF_GRAD + k] = v;
            else atomicAdd(v_rows + (int64_t)s_id[j] * SURF_GRAD + k, v);
        }
        __syncthreads();
    }
}

// ACCUM: v_means holds the SH backward's direction gradient and is added to.
template <bool ACCUM>
__global__ __launch_bounds__(256) void surfel_preprocess_bwd_kernel(
    int N, const float* __restrict__ means, const float* __restrict__ scales, const float* __restrict__ quats,
    const float* __restrict__ viewmatrix, const float* __restrict__ projmatrix, int W, int H, float mod,
    const int32_t* __restrict__ radii, const float* __restrict__ v_rows,
    float* __restrict__ v_means, float* __restrict__ v_scales, float* __restrict__ v_quats, float* __restrict__ v_opac,
    float* __restrict__ v_means2d, float* __restrict__ v_colors_precomp) {
    __shared__ float s_cam[32];
    if (threadIdx.x < 16) { s_cam[threadIdx.x] = viewmatrix[threadIdx.x]; s_cam[16 + threadIdx.x] = projmatrix[threadIdx.x]; }
    __syncthreads();
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= N) return;
    float vp[3] = {0.f, 0.f, 0.f}, vs[2] = {0.f, 0.f}, vq[4] = {0.f, 0.f, 0.f, 0.f}, vo = 0.f, v2[2] = {0.f, 0.f}, vc[3] = {0.f, 0.f, 0.f};
    if (radii[g] > 0) {
        const float* V = s_cam;
        const float p[3] = {means[g * 3 + 0], means[g * 3 + 1], means[g * 3 + 2]};
        const float q[4] = {quats[g * 4 + 0], quats[g * 4 + 1], quats[g * 4 + 2], quats[g * 4 + 3]};
        const float s[2] = {scales[g * 2 + 0], scales[g * 2 + 1]};
        SurfelGeom G;
        surfel_geom(V, s_cam + 16, p, q, s, mod, W, H, G);
        const float* vr = v_rows + (int64_t)g * SURF_GRAD;
        float gTu[3] = {vr[0], vr[1], vr[2]}, gTv[3] = {vr[3], vr[4], vr[5]}, gTw[3] = {vr[6], vr[7], vr[8]};
        const float gcx = vr[9], gcy = vr[10];
        vo = vr[11];
        vc[0] = vr[15]; vc[1] = vr[16]; vc[2] = vr[17];
        // upstream's densification proxy: the compositing's own dL/dTu.z, dL/dTv.z, scaled by the depth and the half image size
        v2[0] = gTu[2] * G.Tw[2] * (0.5f * (float)W);
        v2[1] = gTv[2] * G.Tw[2] * (0.5f * (float)H);
        // centre = (f.(Tu Tw), f.(Tv Tw)), f = t / d, d = t.(Tw Tw)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float fTw = G.f[i] * G.Tw[i];
            gTu[i] += gcx * fTw;
            gTv[i] += gcy * fTw;
            gTw[i] += gcx * (G.f[i] * G.Tu[i] - 2.f * G.cx * fTw) + gcy * (G.f[i] * G.Tv[i] - 2.f * G.cy * fTw);
        }
        // Tu = (t_u.a0, t_v.a0, p.a0 + b0), Tv with a1, Tw with a2
        float gtu[3], gtv[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            gtu[i] = gTu[0] * G.a[0][i] + gTv[0] * G.a[1][i] + gTw[0] * G.a[2][i];
            gtv[i] = gTu[1] * G.a[0][i] + gTv[1] * G.a[1][i] + gTw[1] * G.a[2][i];
            vp[i] = gTu[2] * G.a[0][i] + gTv[2] * G.a[1][i] + gTw[2] * G.a[2][i];
        }
        // view normal = sign (R[:,2] V3)
        float gnw[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) gnw[r] = G.sign * (V[r * 4 + 0] * vr[12] + V[r * 4 + 1] * vr[13] + V[r * 4 + 2] * vr[14]);
        vs[0] = mod * (G.R[0] * gtu[0] + G.R[3] * gtu[1] + G.R[6] * gtu[2]);
        vs[1] = mod * (G.R[1] * gtv[0] + G.R[4] * gtv[1] + G.R[7] * gtv[2]);
        float gR[9];
#pragma unroll
        for (int i = 0; i < 3; ++i) { gR[i * 3 + 0] = G.su * gtu[i]; gR[i * 3 + 1] = G.sv * gtv[i]; gR[i * 3 + 2] = gnw[i]; }
        const float w = G.qn[0], qx = G.qn[1], qy = G.qn[2], qz = G.qn[3];
        float gq[4];
        gq[0] = 2.f * (-qz * gR[1] + qy * gR[2] + qz * gR[3] - qx * gR[5] - qy * gR[6] + qx * gR[7]);
        gq[1] = 2.f * (qy * gR[1] + qz * gR[2] + qy * gR[3] - 2.f * qx * gR[4] - w * gR[5] + qz * gR[6] + w * gR[7] - 2.f * qx * gR[8]);
        gq[2] = 2.f * (-2.f * qy * gR[0] + qx * gR[1] + w * gR[2] + qx * gR[3] + qz * gR[5] - w * gR[6] + qz * gR[7] - 2.f * qy * gR[8]);
        gq[3] = 2.f * (-2.f * qz * gR[0] - w * gR[1] + qx * gR[2] + w * gR[3] - 2.f * qz * gR[4] + qy * gR[5] + qx * gR[6] + qy * gR[7]);
        const float dot = G.qn[0] * gq[0] + G.qn[1] * gq[1] + G.qn[2] * gq[2] + G.qn[3] * gq[3];
        const float iq = 1.f / G.qlen;
#pragma unroll
        for (int j = 0; j < 4; ++j) vq[j] = (gq[j] - G.qn[j] * dot) * iq;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) v_means[g * 3 + i] = ACCUM ? v_means[g * 3 + i] + vp[i] : vp[i];
    v_scales[g * 2 + 0] = vs[0]; v_scales[g * 2 + 1] = vs[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) v_quats[g * 4 + j] = vq[j];
    v_opac[g] = vo;
    v_means2d[g * 3 + 0] = v2[0]; v_means2d[g * 3 + 1] = v2[1]; v_means2d[g * 3 + 2] = 0.f;
    if (v_colors_precomp) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v_colors_precomp[g * 3 + c] = vc[c];
    }
}

struct SurfelGeomLayout { size_t means2d, depths, rec, colors, clamped, order, cum, big_list, spans, total; };
static SurfelGeomLayout surfel_geom_layout(size_t n) {
    SurfelGeomLayout g;
    Carve c;
    g.rec = c.take(4 * SURF_REC * n); g.means2d = c.take(8 * n); g.depths = c.take(4 * n); g.colors = c.take(12 * n); g.clamped = c.take(3 * n);
    g.order = c.take(4 * n); g.cum = c.take(8 * (n + 1)); g.big_list = c.take(4 * n); g.spans = c.take((size_t)GSPL_BIN_SPAN_BYTES * n);
    g.total = c.off;
    return g;
}
struct SurfelImageLayout { size_t final_T, M1, M2, last, median, offsets, total; };
static SurfelImageLayout surfel_image_layout(size_t pixels, size_t tiles) {
    SurfelImageLayout m;
    Carve c;
    m.final_T = c.take(4 * pixels); m.M1 = c.take(4 * pixels); m.M2 = c.take(4 * pixels); m.last = c.take(4 * pixels); m.median = c.take(4 * pixels);
    m.offsets = c.take(4 * (tiles + 1));
    m.total = c.off;
    return m;
}

static void carve_surfel_state(gspl_surfel_state* st, char* geom, const SurfelGeomLayout& g, char* img, const SurfelImageLayout& im) {
    st->rec = (float*)(geom + g.rec); st->means2d = (float*)(geom + g.means2d); st->depths = (float*)(geom + g.depths);
    st->colors = (float*)(geom + g.colors); st->clamped = (uint8_t*)(geom + g.clamped);
    st->final_T = (float*)(img + im.final_T); st->M1 = (float*)(img + im.M1); st->M2 = (float*)(img + im.M2);
    st->last_contrib = (int32_t*)(img + im.last); st->median_contrib = (int32_t*)(img + im.median); st->offsets = (int32_t*)(img + im.offsets);
}

}  // namespace gspl

extern "C" size_t gspl_surfel_state_bytes(void) { return sizeof(gspl_surfel_state); }

extern "C" int gspl_rasterize_surfel_fwd(
    int N, int degree, int n_coeffs,
    const float* means3D, const float* scales, const float* rotations, const float* shs, const float* colors_precomp, const float* opacities,
    const float* viewmatrix, const float* projmatrix, const float* campos, const float* bg,
    int width, int height, float scale_modifier,
    gspl_alloc_fn alloc, void* alloc_ctx,
    float* out_color, float* out_allmap, int32_t* radii, gspl_surfel_state* st, void* stream) {
    using namespace gspl;
    if (N < 0 || width <= 0 || height <= 0 || !alloc || !st || !out_color || !out_allmap || !bg) return fail_arg("rasterize_surfel_fwd: bad argument");
    if (N > 0 && (!means3D || !scales || !rotations || !opacities || !radii || !viewmatrix || !projmatrix)) return fail_arg("rasterize_surfel_fwd: NULL required pointer");
    if (N > 0 && !colors_precomp && (!shs || !campos || degree < 0 || degree > 4 || n_coeffs < (degree + 1) * (degree + 1)))
        return fail_arg("rasterize_surfel_fwd: need shs + campos (and a valid degree / n_coeffs) or colors_precomp");
    const TileGrid grid = tile_grid16(width, height);
    const int tile_w = grid.w, n_tiles = grid.n();
    hipStream_t s = (hipStream_t)stream;
    memset(st, 0, sizeof(*st));
    st->N = N; st->width = width; st->height = height;
    const size_t n = (size_t)(N > 0 ? N : 1);
    const SurfelGeomLayout g = surfel_geom_layout(n);
    const SurfelImageLayout im = surfel_image_layout((size_t)width * height, (size_t)n_tiles);
    char* geom = (char*)alloc(alloc_ctx, GSPL_BUF_GEOMETRY, g.total);
    char* img = (char*)alloc(alloc_ctx, GSPL_BUF_IMAGE, im.total);
    if (!geom || !img) return fail_arg("rasterize_surfel_fwd: allocation call-back returned NULL");
    carve_surfel_state(st, geom, g, img, im);
    int64_t n_isects = 0;
    int rc = GSPL_OK;
    if (N > 0) {
        hipLaunchKernelGGL(surfel_preprocess_fwd_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, means3D, scales, rotations, opacities, viewmatrix,
                           projmatrix, width, height, scale_modifier, colors_precomp, radii, st->means2d, st->depths, st->rec, st->colors);
        rc = check_launch("rasterize_surfel_fwd(preprocess)");
        if (rc != GSPL_OK) return rc;
        if (!colors_precomp) {
            rc = sh_fwd_launch(N, 1, degree, means3D, campos, sh_coeffs(shs, nullptr, n_coeffs), nullptr, radii, GSPL_SH_ADD_HALF_CLAMP, st->colors,
                               st->clamped, stream, nullptr);
            if (rc != GSPL_OK) return rc;
        }
        const size_t ws1_bytes = gspl_bin_workspace_bytes(N, 0);
        void* ws1 = alloc(alloc_ctx, GSPL_BUF_BINNING, ws1_bytes);
        int64_t* host = pinned_words();
        if (!ws1) return fail_arg("rasterize_surfel_fwd: allocation call-back returned NULL");
        if (!host) return fail_arg("rasterize_surfel_fwd: no pinned host word");
        const BinSplats bins{N, GSPL_MODE_INRIA, st->means2d, radii, st->depths, nullptr, nullptr};
        const BinOrder ord{(int32_t*)(geom + g.order), (int64_t*)(geom + g.cum), (int32_t*)(geom + g.big_list), geom + g.spans};
        host[0] = -1;
        rc = bin_count_ticket(bins, grid, ord, host, ws1, ws1_bytes, stream, 0ull);
        // the frame's one read-back: the list length, stored into pinned memory by the scan (also waited for when the count failed: the
        // scan may be in flight, and `host` is the thread's one block)
        const int rc_sync = check_hip(hipStreamSynchronize(s), "rasterize_surfel_fwd: list length");
        if (rc != GSPL_OK) return rc;
        if (rc_sync != GSPL_OK) return rc_sync;
        n_isects = host[0];
        if (n_isects < 0) return fail_arg("rasterize_surfel_fwd: the list length never arrived");
        rc = bin_lists_known(bins, ord, grid, n_isects, alloc, alloc_ctx, &st->flatten_ids, st->offsets, stream, "rasterize_surfel_fwd");
        if (rc != GSPL_OK) return rc;
    }
    st->n_isects = n_isects;
    hipLaunchKernelGGL(surfel_fwd_kernel, dim3(n_tiles), dim3(256), 0, s, width, height, tile_w, n_tiles, n_isects, st->offsets, st->flatten_ids,
                       st->rec, st->colors, bg, out_color, out_allmap, st->final_T, st->M1, st->M2, st->last_contrib, st->median_contrib);
    return check_launch("rasterize_surfel_fwd(composite)");
}

extern "C" int gspl_rasterize_surfel_bwd(
    int degree, int n_coeffs,
    const float* means3D, const float* scales, const float* rotations, const float* shs,
    const float* viewmatrix, const float* projmatrix, const float* campos, const float* bg, float scale_modifier,
    const int32_t* radii, const gspl_surfel_state* st, const float* v_out_color, const float* v_out_allmap,
    gspl_alloc_fn alloc, void* alloc_ctx, float* v_rows,
    float* v_means3D, float* v_means2D, float* v_shs, float* v_colors_precomp, float* v_opacities, float* v_scales, float* v_rotations,
    void* stream) {
    using namespace gspl;
    if (!st || st->N < 0) return fail_arg("rasterize_surfel_bwd: bad state");
    const int N = st->N, width = st->width, height = st->height;
    if (N == 0) return GSPL_OK;
    if (!v_rows || !v_out_color || !v_out_allmap || !v_means3D || !v_means2D || !v_opacities || !v_scales || !v_rotations || !bg || !radii ||
        !means3D || !scales || !rotations || !viewmatrix || !projmatrix)
        return fail_arg("rasterize_surfel_bwd: NULL required pointer");
    if ((v_shs == nullptr) == (v_colors_precomp == nullptr)) return fail_arg("rasterize_surfel_bwd: exactly one of v_shs and v_colors_precomp");
    if (v_shs && (!shs || !campos || degree < 0 || degree > 4 || n_coeffs < (degree + 1) * (degree + 1))) return fail_arg("rasterize_surfel_bwd: shs / campos / degree");
    const int tile_w = (width + 15) / 16, tile_h = (height + 15) / 16, n_tiles = tile_w * tile_h;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(v_rows, 0, (size_t)N * SURF_GRAD * sizeof(float), s);
    if (e != hipSuccess) return check_hip(e, "rasterize_surfel_bwd: clear");
    int rc = GSPL_OK;
    const int64_t n_isects = st->n_isects;
    if (n_isects > 0) {
        const bool ordered = gspl_get_deterministic() != 0;
        float* entries = nullptr;
        if (ordered) {
            if (!alloc) return fail_arg("rasterize_surfel_bwd: the deterministic mode needs the allocation call-back");
            entries = (float*)alloc(alloc_ctx, GSPL_BUF_SURFEL_ENTRIES, ordered_scratch(N, n_isects, SURF_GRAD).total);
            if (!entries) return fail_arg("rasterize_surfel_bwd: allocation call-back returned NULL");
            e = hipMemsetAsync(entries, 0, (size_t)n_isects * SURF_GRAD * sizeof(float), s);
            if (e != hipSuccess) return check_hip(e, "rasterize_surfel_bwd: clear");
        }
        hipLaunchKernelGGL(surfel_bwd_kernel, dim3(n_tiles), dim3(256), 0, s, width, height, tile_w, n_tiles, n_isects, st->offsets, st->flatten_ids,
                           st->rec, st->colors, bg, st->final_T, st->M1, st->M2, st->last_contrib, st->median_contrib, v_out_color, v_out_allmap,
                           v_rows, entries);
        rc = check_launch("rasterize_surfel_bwd(composite)");
        if (rc != GSPL_OK) return rc;
        if (ordered) {      // (v_rows is clear: the sums land as they are)
            rc = ordered_reduce(N, n_isects, SURF_GRAD, st->flatten_ids, entries, v_rows, SURF_GRAD, s, "rasterize_surfel_bwd(ordered reduce)");
            if (rc != GSPL_OK) return rc;
        }
    }
    bool accum = false;
    if (v_shs) {
        rc = sh_bwd_launch(N, 1, degree, n_coeffs, means3D, campos, sh_coeffs(shs, nullptr, n_coeffs), nullptr, radii, GSPL_SH_ADD_HALF_CLAMP, st->clamped,
                           v_rows + 15, SURF_GRAD, sh_grads(v_shs, nullptr), v_means3D, stream, nullptr, nullptr);
        if (rc != GSPL_OK) return rc;
        accum = true;
    }
    const dim3 grid((N + 255) / 256);
    if (accum)
        hipLaunchKernelGGL(surfel_preprocess_bwd_kernel<true>, grid, dim3(256), 0, s, N, means3D, scales, rotations, viewmatrix, projmatrix, width, height,
                           scale_modifier, radii, v_rows, v_means3D, v_scales, v_rotations, v_opacities, v_means2D, v_colors_precomp);
    else
        hipLaunchKernelGGL(surfel_preprocess_bwd_kernel<false>, grid, dim3(256), 0, s, N, means3D, scales, rotations, viewmatrix, projmatrix, width, height,
                           scale_modifier, radii, v_rows, v_means3D, v_scales, v_rotations, v_opacities, v_means2D, v_colors_precomp);
    return check_launch("rasterize_surfel_bwd(preprocess)");
}

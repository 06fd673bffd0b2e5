// mesh.hip — 2DGS mesh extraction: TSDF fusion of depth maps and marching tetrahedra (gfx950, wave64); include/gspl_hip.h section 18.
//
// What 2DGS's `extract_mesh_unbounded` (Huang et al., "2D Gaussian Splatting for Geometrically Accurate Radiance Fields") does with some
// twenty elementwise / grid_sample launches and four masked scatters per camera and chunk, and a marching cubes on the CPU:
//   * tsdf_fuse_kernel: one thread per sample, the V views in a loop, the sample's running average (tsdf, weight, colour) in registers
//     from the first view to the last: the state is read once and written once per call whatever V is.  The sample is either a row of
//     `points` or a node of a lattice that is never materialised (k fastest: the 64 lanes of a wave are neighbours along k, their taps
//     neighbours in the map).  The view matrices are indexed by the loop counter alone: wave-uniform (scalar) loads.  The geometry of a
//     view (contraction, projection, pixel, bilinear weights, sdf / sdf_trunc) is evaluated in fp64 from the fp32 inputs and rounded
//     once: a few dozen fp64 operations per view next to four to sixteen cache-served taps; the running average itself is fp32, because
//     its state is, so that a call over views [0, a) followed by one over [a, V) gives the bits of one call.
//   * mtet_count_kernel / mtet_emit_kernel: one thread per cell, the six Kuhn tetrahedra in a fixed order.  A cell whose eight corners
//     lie on one side of the level is done after eight loads.  No case table: the triangles follow from a stable partition of the four
//     corners, and their orientation from an exact integer test on the corner offsets.
// No atomics; every result is bit-reproducible.  (No LDS in the source; the compiler keeps the emit kernel's small per-thread arrays
// in 9 KB of it: profiles/mesh_kernel_resources.txt.)
#include "gspl_device.h"
#include "gspl_host.h"

namespace gspl {
namespace {

constexpr int kT = 256;

// the device table of gspl_tsdf_fuse (GSPL_TSDF_TABLE_FLOATS floats)
enum { kCenter = 0, kRadius = 3, kVoxel = 4, kSdfTrunc = 5, kDepthTrunc = 6, kContract = 7, kWithRgb = 8, kLo = 9, kHi = 12 };

struct Lattice { int n[3], b[3], m[3]; };

// bilinear taps of a pixel in (-1, 1)^2: align_corners=True, border padding
struct Taps {
    int64_t o00, o01, o10, o11;
    double w00, w01, w10, w11;
};

__device__ inline Taps taps_of(double px, double py, int H, int W) {
    const double ix = fmin(fmax((px + 1.0) * 0.5 * (double)(W - 1), 0.0), (double)(W - 1));
    const double iy = fmin(fmax((py + 1.0) * 0.5 * (double)(H - 1), 0.0), (double)(H - 1));
    const int x0 = min(max((int)floor(ix), 0), W - 1), y0 = min(max((int)floor(iy), 0), H - 1);
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const double fx = ix - (double)x0, fy = iy - (double)y0;
    Taps t;
    t.o00 = (int64_t)y0 * W + x0;
    t.o01 = (int64_t)y0 * W + x1;
    t.o10 = (int64_t)y1 * W + x0;
    t.o11 = (int64_t)y1 * W + x1;
    t.w00 = (1.0 - fx) * (1.0 - fy);
    t.w01 = fx * (1.0 - fy);
    t.w10 = (1.0 - fx) * fy;
    t.w11 = fx * fy;
    return t;
}

__device__ inline double sample(const float* __restrict__ map, const Taps& t) {
    return (double)map[t.o00] * t.w00 + (double)map[t.o01] * t.w01 + (double)map[t.o10] * t.w10 + (double)map[t.o11] * t.w11;
}

template <bool LATTICE, bool RGB>
__global__ __launch_bounds__(kT) void tsdf_fuse_kernel(int64_t M, const float* __restrict__ points, Lattice L, const float* __restrict__ table,
                                                       int V, int H, int W, const float* __restrict__ views, const float* __restrict__ depth,
                                                       const float* __restrict__ rgb, float* __restrict__ tsdf, float* __restrict__ weight,
                                                       float* __restrict__ color) {
    const int64_t idx = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (idx >= M) return;
    float s[3];
    if (LATTICE) {
        const int64_t plane = (int64_t)L.m[1] * L.m[2];
        const int g[3] = {L.b[0] + (int)(idx / plane), L.b[1] + (int)((idx % plane) / L.m[2]), L.b[2] + (int)(idx % L.m[2])};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float lo = table[kLo + a], hi = table[kHi + a];
            s[a] = L.n[a] > 1 ? fmaf((float)g[a], __fdiv_rn(__fsub_rn(hi, lo), (float)(L.n[a] - 1)), lo) : lo;
        }
    } else {
#pragma unroll
        for (int a = 0; a < 3; ++a) s[a] = points[idx * 3 + a];
    }
    const bool with_rgb = RGB && table[kWithRgb] != 0.f;
    const double voxel = (double)table[kVoxel];
    double trunc = table[kSdfTrunc] > 0.f ? (double)table[kSdfTrunc] : 5.0 * voxel;
    const double depth_trunc = (double)table[kDepthTrunc];
    double x[3] = {(double)s[0], (double)s[1], (double)s[2]};
    if (table[kContract] != 0.f) {
        const double mag = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
        if (mag > 1.0) trunc *= 1.0 / (2.0 - fmin(mag, 1.9));
        const double radius = (double)table[kRadius];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double u = mag < 1.0 ? x[a] : (1.0 / (2.0 - mag)) * (x[a] / mag);
            x[a] = u * radius + (double)table[kCenter + a];
        }
    }
    float f = tsdf[idx], w = weight[idx];
    float c[3] = {0.f, 0.f, 0.f};
    if (with_rgb) {
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = color[idx * 3 + a];
    }
    const int64_t HW = (int64_t)H * W;
    for (int v = 0; v < V; ++v) {
        const float* __restrict__ P = views + (int64_t)v * 16;      // wave-uniform
        const double pw = x[0] * (double)P[3] + x[1] * (double)P[7] + x[2] * (double)P[11] + (double)P[15];
        const double nx = x[0] * (double)P[0] + x[1] * (double)P[4] + x[2] * (double)P[8] + (double)P[12];
        const double ny = x[0] * (double)P[1] + x[1] * (double)P[5] + x[2] * (double)P[9] + (double)P[13];
        // Most views miss most samples: |n| > w can only give a quotient that rounds to 1 or more, so those leave before the two
        // divisions.  (NaN fails every comparison: such a view does not count and nothing is read.)
        if (!(pw > 0.0 && fabs(nx) <= pw && fabs(ny) <= pw)) continue;
        const double px = nx / pw, py = ny / pw;
        if (!(px > -1.0 && px < 1.0 && py > -1.0 && py < 1.0)) continue;
        const Taps t = taps_of(px, py, H, W);
        const double d = sample(depth + (int64_t)v * HW, t);
        const double sdf = d - pw;
        if (!(sdf > -trunc)) continue;
        if (depth_trunc > 0.0 && !(d > 0.0 && d <= depth_trunc)) continue;
        const float val = (float)fmin(fmax(sdf / trunc, -1.0), 1.0);
        const float w1 = w + 1.f;
        f = __fdiv_rn(fmaf(f, w, val), w1);
        if (with_rgb) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float ca = (float)sample(rgb + ((int64_t)v * 3 + a) * HW, t);
                c[a] = __fdiv_rn(fmaf(c[a], w, ca), w1);
            }
        }
        w = w1;
    }
    tsdf[idx] = f;
    weight[idx] = w;
    if (with_rgb) {
#pragma unroll
        for (int a = 0; a < 3; ++a) color[idx * 3 + a] = c[a];
    }
}

// ---- marching tetrahedra ---------------------------------------------------------------------------------------------------------------
// A cell corner is a 3-bit mask: bit 2 = +1 along axis 0 (i, the slowest), bit 1 along axis 1 (j), bit 0 along axis 2 (k).  The six Kuhn
// tetrahedra, one per permutation (a, b, c) of the axes in lexicographic order: corners 0, e_a, e_a + e_b, 7, packed three bits each.
__host__ __device__ constexpr int axis_bit(int a) { return 4 >> a; }
__host__ __device__ constexpr int tet_pack(int a, int b) { return (axis_bit(a) << 3) | ((axis_bit(a) | axis_bit(b)) << 6) | (7 << 9); }
constexpr int kTets[6] = {tet_pack(0, 1), tet_pack(0, 2), tet_pack(1, 0), tet_pack(1, 2), tet_pack(2, 0), tet_pack(2, 1)};

struct Cell {
    float f[8];
    int inside;         // bit c: corner c is inside
};

__device__ inline Cell load_cell(const float* __restrict__ vol, int Y, int Z, int i, int j, int k, float level) {
    Cell c;
    c.inside = 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        c.f[m] = vol[((int64_t)(i + (m >> 2)) * Y + (j + ((m >> 1) & 1))) * Z + (k + (m & 1))];
        c.inside |= (c.f[m] < level ? 1 : 0) << m;
    }
    return c;
}

// the four corners of tetrahedron `pack` in its own order: bit t of the result = corner t is inside
__device__ inline int tet_inside(int inside, int pack) {
    int bits = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) bits |= ((inside >> ((pack >> (3 * t)) & 7)) & 1) << t;
    return bits;
}

__device__ inline int tet_triangles(int bits) {
    const int k = __popc(bits);
    return k == 0 || k == 4 ? 0 : (k == 2 ? 2 : 1);
}

__device__ inline int cell_triangles(int inside) {
    if (inside == 0 || inside == 255) return 0;
    int n = 0;
#pragma unroll
    for (int q = 0; q < 6; ++q) n += tet_triangles(tet_inside(inside, kTets[q]));
    return n;
}

__device__ inline float pick8(const float f[8], int m) {
    float r = f[0];
#pragma unroll
    for (int c = 1; c < 8; ++c) r = m == c ? f[c] : r;
    return r;
}

struct EmitArgs {
    int Y, Z;
    int g[3], b[3];
    float level;
};

// One vertex: the edge between tetrahedron corners ta < tb (positions in the tetrahedron's order, which is the order of the global
// linear index).  Returns the key; p receives the position.
__device__ inline int64_t edge_vertex(const Cell& c, int pack, int ta, int tb, const int cell[3], const EmitArgs& A, const float* __restrict__ grid,
                                      float p[3]) {
    const int ma = (pack >> (3 * ta)) & 7, mb = (pack >> (3 * tb)) & 7;
    const float fa = pick8(c.f, ma), fb = pick8(c.f, mb);
    const float t = __fdiv_rn(__fsub_rn(A.level, fa), __fsub_rn(fb, fa));
    const int d = ma ^ mb;      // mb contains ma: the set bits are the axes the edge runs along
    int ga[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        ga[a] = A.b[a] + cell[a] + ((ma >> (2 - a)) & 1);
        const float step = grid[3 + a], origin = grid[a];
        const float pa = fmaf((float)ga[a], step, origin);      // the node as gspl_tsdf_fuse's lattice places it
        const float pb = fmaf((float)(ga[a] + ((d >> (2 - a)) & 1)), step, origin);
        p[a] = fmaf(t, __fsub_rn(pb, pa), pa);
    }
    // direction: x 0, y 1, z 2, xy 3, xz 4, yz 5, xyz 6   (d = 4 x + 2 y + z)
    const int dir = d == 4 ? 0 : d == 2 ? 1 : d == 1 ? 2 : d == 6 ? 3 : d == 5 ? 4 : d == 3 ? 5 : 6;
    return ((((int64_t)ga[0] * A.g[1]) + ga[1]) * A.g[2] + ga[2]) * 8 + dir;
}

__device__ inline void corner_offset(int m, int o[3]) {
    o[0] = (m >> 2) & 1;
    o[1] = (m >> 1) & 1;
    o[2] = m & 1;
}

// Writes the triangles of one tetrahedron at `out` (in triangles); returns how many.
__device__ inline int emit_tet(const Cell& c, int pack, const int cell[3], const EmitArgs& A, const float* __restrict__ grid, int64_t out,
                               float* __restrict__ vertices, int64_t* __restrict__ keys) {
    const int bits = tet_inside(c.inside, pack);
    const int k = __popc(bits);
    if (k == 0 || k == 4) return 0;
    // stable partition: names 0..3 -> positions in the tetrahedron, inside corners first; two bits each
    int q = 0, n = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) if ((bits >> t) & 1) { q |= t << (2 * n); ++n; }
#pragma unroll
    for (int t = 0; t < 4; ++t) if (!((bits >> t) & 1)) { q |= t << (2 * n); ++n; }
    // k_out * sum of the inside offsets - k_in * sum of the outside offsets: (centroid inside - centroid outside) k_in k_out
    int dvec[3] = {0, 0, 0};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        int o[3];
        corner_offset((pack >> (3 * t)) & 7, o);
        const int wgt = ((bits >> t) & 1) ? 4 - k : -k;
#pragma unroll
        for (int a = 0; a < 3; ++a) dvec[a] += wgt * o[a];
    }
    // edges as pairs of names, four bits each (first name in the high two), three per triangle
    //   k = 1: (0,1) (0,2) (0,3)      k = 3: (0,3) (1,3) (2,3)      k = 2: (0,2) (0,3) (1,3)  then  (0,2) (1,3) (1,2)
    const int first = k == 1 ? 0x123 : (k == 3 ? 0x37B : 0x237);
    const int second = 0x276;
    const int ntri = k == 2 ? 2 : 1;
    for (int tri = 0; tri < ntri; ++tri) {
        const int edges = tri == 0 ? first : second;
        float p[3][3];
        int64_t key[3];
        int twice[3][3];        // the edge midpoints times two, as corner offsets
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int pair = (edges >> (4 * (2 - e))) & 15;
            const int t0 = (q >> (2 * (pair >> 2))) & 3, t1 = (q >> (2 * (pair & 3))) & 3;
            const int ta = min(t0, t1), tb = max(t0, t1);
            key[e] = edge_vertex(c, pack, ta, tb, cell, A, grid, p[e]);
            int oa[3], ob[3];
            corner_offset((pack >> (3 * ta)) & 7, oa);
            corner_offset((pack >> (3 * tb)) & 7, ob);
#pragma unroll
            for (int a = 0; a < 3; ++a) twice[e][a] = oa[a] + ob[a];
        }
        int u[3], w[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            u[a] = twice[1][a] - twice[0][a];
            w[a] = twice[2][a] - twice[0][a];
        }
        const int dot = (u[1] * w[2] - u[2] * w[1]) * dvec[0] + (u[2] * w[0] - u[0] * w[2]) * dvec[1] + (u[0] * w[1] - u[1] * w[0]) * dvec[2];
        const bool flip = dot > 0;      // the normal points from the outside corners towards the inside ones
        const int64_t base = (out + tri) * 3;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int src = e == 0 ? 0 : (flip ? 3 - e : e);
            float ps[3];
            int64_t ks;
            // (src is 0, 1 or 2: selected without a run-time index)
#pragma unroll
            for (int a = 0; a < 3; ++a) ps[a] = src == 0 ? p[0][a] : (src == 1 ? p[1][a] : p[2][a]);
            ks = src == 0 ? key[0] : (src == 1 ? key[1] : key[2]);
#pragma unroll
            for (int a = 0; a < 3; ++a) vertices[(base + e) * 3 + a] = ps[a];
            keys[base + e] = ks;
        }
    }
    return ntri;
}

__device__ inline bool cell_of(int64_t idx, int X, int Y, int Z, int cell[3]) {
    const int64_t cz = Z - 1, cy = Y - 1;
    if (idx >= (int64_t)(X - 1) * cy * cz) return false;
    cell[2] = (int)(idx % cz);
    cell[1] = (int)((idx / cz) % cy);
    cell[0] = (int)(idx / (cz * cy));
    return true;
}

__global__ __launch_bounds__(kT) void mtet_count_kernel(int X, int Y, int Z, const float* __restrict__ vol, float level, uint8_t* __restrict__ counts) {
    const int64_t idx = (int64_t)blockIdx.x * kT + threadIdx.x;
    int cell[3];
    if (!cell_of(idx, X, Y, Z, cell)) return;
    counts[idx] = (uint8_t)cell_triangles(load_cell(vol, Y, Z, cell[0], cell[1], cell[2], level).inside);
}

__global__ __launch_bounds__(kT) void mtet_emit_kernel(int X, int Y, int Z, const float* __restrict__ vol, EmitArgs A, const float* __restrict__ grid,
                                                       const int32_t* __restrict__ offsets, int64_t total, float* __restrict__ vertices,
                                                       int64_t* __restrict__ keys) {
    const int64_t idx = (int64_t)blockIdx.x * kT + threadIdx.x;
    int cell[3];
    if (!cell_of(idx, X, Y, Z, cell)) return;
    const Cell c = load_cell(vol, Y, Z, cell[0], cell[1], cell[2], A.level);
    const int n = cell_triangles(c.inside);
    if (n == 0) return;
    int64_t out = offsets[idx];
    if (out < 0 || out + n > total) return;      // offsets that are not this volume's prefix sum: nothing is written out of bounds
#pragma unroll
    for (int q = 0; q < 6; ++q) out += emit_tet(c, kTets[q], cell, A, grid, out, vertices, keys);
}

inline bool grid_fits(int64_t n) { return (n + kT - 1) / kT <= 2147483647LL; }

}  // namespace
}  // namespace gspl

extern "C" int gspl_tsdf_fuse(int64_t M, const float* points, int n0, int n1, int n2, int b0, int b1, int b2, int m0, int m1, int m2,
                              const float* table, int V, int H, int W, const float* view_table, const float* depth, const float* rgb,
                              float* tsdf, float* weight, float* color, void* stream) {
    using namespace gspl;
    if (M < 0 || V < 0) return fail_arg("tsdf_fuse: M and V must not be negative");
    if (M == 0 || V == 0) return GSPL_OK;
    if (H < 1 || W < 1) return fail_arg("tsdf_fuse: H and W must be at least 1");
    if (!grid_fits(M)) return fail_arg("tsdf_fuse: M too large for one launch (M <= 2^39)");
    if (!table || !view_table || !depth || !tsdf || !weight) return fail_arg("tsdf_fuse: NULL pointer");
    Lattice L{{n0, n1, n2}, {b0, b1, b2}, {m0, m1, m2}};
    if (!points) {
        for (int a = 0; a < 3; ++a)
            if (L.n[a] < 1 || L.m[a] < 1 || L.b[a] < 0 || (int64_t)L.b[a] + L.m[a] > L.n[a])
                return fail_arg("tsdf_fuse: lattice mode needs n >= 1 and a block 0 <= b, b + m <= n on every axis");
        if ((int64_t)m0 * m1 * m2 != M) return fail_arg("tsdf_fuse: lattice mode needs M == m0 m1 m2");
    }
    const bool with_rgb = rgb != nullptr && color != nullptr;
    const dim3 grid((unsigned)((M + kT - 1) / kT)), block(kT);
    hipStream_t s = (hipStream_t)stream;
#define GSPL_FUSE(LAT, RGB) hipLaunchKernelGGL((tsdf_fuse_kernel<LAT, RGB>), grid, block, 0, s, M, points, L, table, V, H, W, view_table, depth, rgb, tsdf, weight, color)
    if (points) { if (with_rgb) GSPL_FUSE(false, true); else GSPL_FUSE(false, false); }
    else { if (with_rgb) GSPL_FUSE(true, true); else GSPL_FUSE(true, false); }
#undef GSPL_FUSE
    return check_launch("tsdf_fuse");
}

extern "C" int gspl_mtet_count(int X, int Y, int Z, const float* volume, float level, uint8_t* counts, void* stream) {
    using namespace gspl;
    if (X < 0 || Y < 0 || Z < 0) return fail_arg("mtet_count: negative volume shape");
    if (X < 2 || Y < 2 || Z < 2) return GSPL_OK;
    const int64_t cells = (int64_t)(X - 1) * (Y - 1) * (Z - 1);
    if (!grid_fits(cells)) return fail_arg("mtet_count: volume too large for one launch");
    if (!volume || !counts) return fail_arg("mtet_count: NULL pointer");
    hipLaunchKernelGGL(mtet_count_kernel, dim3((unsigned)((cells + kT - 1) / kT)), dim3(kT), 0, (hipStream_t)stream, X, Y, Z, volume, level, counts);
    return check_launch("mtet_count");
}

extern "C" int gspl_mtet_emit(int X, int Y, int Z, const float* volume, float level, const float* grid, int g0, int g1, int g2,
                              int b0, int b1, int b2, const int32_t* offsets, int64_t total, float* vertices, int64_t* keys, void* stream) {
    using namespace gspl;
    if (X < 0 || Y < 0 || Z < 0 || total < 0) return fail_arg("mtet_emit: negative volume shape or total");
    if (X < 2 || Y < 2 || Z < 2 || total == 0) return GSPL_OK;
    const int64_t cells = (int64_t)(X - 1) * (Y - 1) * (Z - 1);
    if (!grid_fits(cells) || cells * 12 > 2147483647LL) return fail_arg("mtet_emit: volume too large (12 triangles per cell must fit 31 bits)");
    if (b0 < 0 || b1 < 0 || b2 < 0 || (int64_t)b0 + X > g0 || (int64_t)b1 + Y > g1 || (int64_t)b2 + Z > g2)
        return fail_arg("mtet_emit: the block must lie inside the global lattice (0 <= b, b + shape <= g)");
    if (!volume || !grid || !offsets || !vertices || !keys) return fail_arg("mtet_emit: NULL pointer");
    EmitArgs A{Y, Z, {g0, g1, g2}, {b0, b1, b2}, level};
    hipLaunchKernelGGL(mtet_emit_kernel, dim3((unsigned)((cells + kT - 1) / kT)), dim3(kT), 0, (hipStream_t)stream, X, Y, Z, volume, A, grid, offsets,
                       total, vertices, keys);
    return check_launch("mtet_emit");
}

// lod.hip — the per-frame front of the partition-LoD route: level selection and the segmented copy of the chosen levels (gfx950;
// include/gspl_hip.h section 26).
//
// Restates internal/renderers/partition_lod_renderer.py `PartitionLoDRendererModule.forward`, lines 550-625: `get_partition_distances`,
// the threshold rule, the frustum test of the visibility filter and the concatenation of the chosen models' five property arrays.
// The reference does this with torch ops, pytorch3d's box overlap, two host waits for the comparison with the previous frame and,
// when the selection changed, a Python loop over the partitions with one `.item()` each and five `torch.concat` over P tensors.
// Here: ONE launch that selects (a single workgroup looping over P; P is a few hundred) and leaves a 16-byte record for the host,
// and ONE launch that copies.
//
// The copy is HBM-bound: 4 (3 + 3K + 1 + 3 + 4) bytes read and written per row.  A workgroup owns a window of GATHER_CHUNK floats of
// ONE destination array, finds the segment of its first row by binary search in dst_start and walks on from there; within a segment
// source and destination are both contiguous, so consecutive lanes touch consecutive addresses on either side.  Where the source
// offset, the destination offset and the length of a piece are all multiples of four floats the piece moves in 16-byte accesses:
// that is every piece of `rotations` (16-byte rows) and of `shs` when K is a multiple of 4 (192-byte rows at degree 3), 208 of the
// 236 bytes of a row.  The 12- and 4-byte-row arrays start a segment on any 16-byte phase, the source's and the destination's
// independent of each other; they move one float per lane (still whole 256-byte lines per wave instruction) rather than through a
// head / realigned body / tail.  No atomics, no scratch: two runs give the same bits.
#pragma clang fp contract(off)
#include "gspl_host.h"
#include "gspl_lod_index.h"

namespace gspl {

static constexpr int LOD_BLOCK = 256;
static constexpr int LOD_MAX_PARTITIONS = GSPL_LOD_MAX_PARTITIONS;
static constexpr int LOD_MAX_LEVELS = GSPL_LOD_MAX_LEVELS;
static constexpr int LOD_BOX_STRIDE = 25;                 // 8 corners x 3 floats per lane, odd: lane r's row on its own banks
static constexpr int64_t GATHER_CHUNK = 4096;             // floats of one destination array per workgroup (16 KiB)
static constexpr float LOD_NEAR = 0.1f, LOD_FAR_FACTOR = 10.f;
static constexpr float LOD_DEGENERATE = 1e-12f;           // an axis is skipped when |a x b|^2 <= this * |a|^2 |b|^2

// ---- the separating-axis test between two convex hexahedra, corners in the reference's order: 0 .. 3 one face clockwise, 4 .. 7 the
// opposite face, corner i + 4 across the edge from corner i -----------------------------------------------------------------------
__host__ __device__ __forceinline__ void hex_face(int f, int& a, int& b, int& c, int& d) {
    if (f == 0) { a = 0; b = 1; c = 2; d = 3; }
    else if (f == 1) { a = 4; b = 5; c = 6; d = 7; }
    else { a = f - 2; b = (f - 1) & 3; c = b + 4; d = a + 4; }
}
// the face's normal as the cross product of its diagonals, and the product of their squared lengths
__host__ __device__ __forceinline__ void hex_normal(const float* V, int f, float& nx, float& ny, float& nz, float& scale) {
    int a, b, c, d;
    hex_face(f, a, b, c, d);
    const float ux = V[c * 3] - V[a * 3], uy = V[c * 3 + 1] - V[a * 3 + 1], uz = V[c * 3 + 2] - V[a * 3 + 2];
    const float vx = V[d * 3] - V[b * 3], vy = V[d * 3 + 1] - V[b * 3 + 1], vz = V[d * 3 + 2] - V[b * 3 + 2];
    nx = uy * vz - uz * vy; ny = uz * vx - ux * vz; nz = ux * vy - uy * vx;
    scale = (ux * ux + uy * uy + uz * uz) * (vx * vx + vy * vy + vz * vz);
}
// the six edge directions: two of face 0 .. 3 (its opposite face's are parallel to them in a frustum and in a box) and the four
// edges between the faces
__host__ __device__ __forceinline__ void hex_edge(const float* V, int e, float& x, float& y, float& z) {
    const int a = e == 0 ? 0 : (e == 1 ? 1 : e - 2), b = e == 0 ? 1 : (e == 1 ? 2 : e + 2);
    x = V[b * 3] - V[a * 3]; y = V[b * 3 + 1] - V[a * 3 + 1]; z = V[b * 3 + 2] - V[a * 3 + 2];
}
// The gap between the two solids' shadows on the axis n (|n|^2 = n2 > 0), in units of length: >= 0 separates
__host__ __device__ __forceinline__ float axis_gap(const float* A, const float* B, float nx, float ny, float nz, float n2) {
    float alo = INFINITY, ahi = -INFINITY, blo = INFINITY, bhi = -INFINITY;
    for (int k = 0; k < 8; ++k) {
        const float a = A[k * 3] * nx + A[k * 3 + 1] * ny + A[k * 3 + 2] * nz;
        const float b = B[k * 3] * nx + B[k * 3 + 1] * ny + B[k * 3 + 2] * nz;
        alo = fminf(alo, a); ahi = fmaxf(ahi, a); blo = fminf(blo, b); bhi = fmaxf(bhi, b);
    }
    return fmaxf(alo - bhi, blo - ahi) / sqrtf(n2);
}
// the largest gap over the 6 + 6 face normals and the 6 x 6 edge cross products (-inf when every axis is degenerate)
__host__ __device__ inline float hex_separation(const float* A, const float* B) {
    float sep = -INFINITY;
    for (int f = 0; f < 12; ++f) {
        float nx, ny, nz, scale;
        hex_normal(f < 6 ? A : B, f < 6 ? f : f - 6, nx, ny, nz, scale);
        const float n2 = nx * nx + ny * ny + nz * nz;
        if (n2 > LOD_DEGENERATE * scale) sep = fmaxf(sep, axis_gap(A, B, nx, ny, nz, n2));
    }
    for (int i = 0; i < 6; ++i) {
        float ax, ay, az;
        hex_edge(A, i, ax, ay, az);
        const float a2 = ax * ax + ay * ay + az * az;
        for (int j = 0; j < 6; ++j) {
            float bx, by, bz;
            hex_edge(B, j, bx, by, bz);
            const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
            const float n2 = nx * nx + ny * ny + nz * nz;
            if (n2 > LOD_DEGENERATE * (a2 * (bx * bx + by * by + bz * bz))) sep = fmaxf(sep, axis_gap(A, B, nx, ny, nz, n2));
        }
    }
    return sep;
}

// One workgroup.  Pass 1: distance, level, the largest distance and the nearest partition; pass 2 (filter on): the frustum test;
// pass 3: the exclusive scan of the chosen lengths.  Thread t owns partitions t, t + 256, ... in every pass.
__global__ __launch_bounds__(LOD_BLOCK) void lod_select_kernel(
    int P, int L, const float* __restrict__ camera_center, const float* __restrict__ transform, const float* __restrict__ box_min,
    const float* __restrict__ box_max, const float* __restrict__ thresholds, const float* __restrict__ boxes3d,
    const float* __restrict__ world_to_camera, const float* __restrict__ K, int width, int height, int visibility_filter,
    const int64_t* __restrict__ seg_start, const int8_t* __restrict__ prev_lod, const uint8_t* __restrict__ prev_visible,
    float* __restrict__ distance, int8_t* __restrict__ lod, uint8_t* __restrict__ visible, int64_t* __restrict__ dst_start,
    int64_t* __restrict__ record) {
    __shared__ float s_box[LOD_BLOCK * LOD_BOX_STRIDE];
    __shared__ float s_frustum[24];
    __shared__ float s_max[LOD_BLOCK / 64], s_min[LOD_BLOCK / 64];
    __shared__ int s_arg[LOD_BLOCK / 64];
    __shared__ long long s_sum[LOD_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // p = (c @ T)[:2]
    const float c0 = camera_center[0], c1 = camera_center[1], c2 = camera_center[2];
    const float px = c0 * transform[0] + c1 * transform[3] + c2 * transform[6];
    const float py = c0 * transform[1] + c1 * transform[4] + c2 * transform[7];

    int differs = 0;
    float dmax = 0.f, dmin = INFINITY;
    int imin = 0x7fffffff;
    for (int p = tid; p < P; p += LOD_BLOCK) {
        const float dx = fmaxf(fmaxf(box_min[p * 2] - px, px - box_max[p * 2]), 0.f);
        const float dy = fmaxf(fmaxf(box_min[p * 2 + 1] - py, py - box_max[p * 2 + 1]), 0.f);
        const float d = sqrtf(dx * dx + dy * dy);
        distance[p] = d;
        int level = L - 1;
        for (int i = L - 2; i >= 0; --i)
            if (d < thresholds[i]) level = i;
        lod[p] = (int8_t)level;
        differs |= level != (int)prev_lod[p];
        dmax = fmaxf(dmax, d);
        if (d < dmin) { dmin = d; imin = p; }           // (p rises: the first of equal distances stays)
    }

    if (visibility_filter) {
        for (int off = 32; off > 0; off >>= 1) {
            dmax = fmaxf(dmax, __shfl_xor(dmax, off, 64));
            const float od = __shfl_xor(dmin, off, 64);
            const int oi = __shfl_xor(imin, off, 64);
            if (od < dmin || (od == dmin && oi < imin)) { dmin = od; imin = oi; }
        }
        if (lane == 0) { s_max[wave] = dmax; s_min[wave] = dmin; s_arg[wave] = imin; }
        __syncthreads();
        dmax = s_max[0]; dmin = s_min[0]; imin = s_arg[0];
        for (int w = 1; w < LOD_BLOCK / 64; ++w) {
            dmax = fmaxf(dmax, s_max[w]);
            if (s_min[w] < dmin || (s_min[w] == dmin && s_arg[w] < imin)) { dmin = s_min[w]; imin = s_arg[w]; }
        }
        // the frustum in camera space: the image corners through K^-1, the near face at 0.1, the far face at 10 max(distance)
        if (tid < 8) {
            const int q = tid & 3;
            const float u = (q == 1 || q == 2) ? (float)width : 0.f, v = q >= 2 ? (float)height : 0.f;
            const float depth = tid < 4 ? LOD_NEAR : LOD_FAR_FACTOR * dmax;
            s_frustum[tid * 3 + 0] = (u - K[2]) / K[0] * depth;
            s_frustum[tid * 3 + 1] = (v - K[5]) / K[4] * depth;
            s_frustum[tid * 3 + 2] = depth;
        }
        __syncthreads();
        float* mine = s_box + tid * LOD_BOX_STRIDE;
        const float* w2c = world_to_camera;               // row-vector convention: x_cam = x_world @ w2c[:3, :3] + w2c[3, :3]
        for (int p = tid; p < P; p += LOD_BLOCK) {
            const float* b = boxes3d + (int64_t)p * 24;
            for (int k = 0; k < 8; ++k) {
                const float x = b[k * 3], y = b[k * 3 + 1], z = b[k * 3 + 2];
                for (int j = 0; j < 3; ++j) mine[k * 3 + j] = x * w2c[j] + y * w2c[4 + j] + z * w2c[8 + j] + w2c[12 + j];
            }
            const int seen = hex_separation(s_frustum, mine) < 0.f || p == imin;
            visible[p] = (uint8_t)seen;
            differs |= seen != (int)prev_visible[p];
        }
    } else {
        for (int p = tid; p < P; p += LOD_BLOCK) {
            visible[p] = 1;
            differs |= prev_visible[p] != 1;
        }
    }
    const int changed = __syncthreads_or(differs);

    long long carry = 0;
    for (int base = 0; base < P; base += LOD_BLOCK) {
        const int p = base + tid;
        long long len = 0;
        if (p < P && visible[p]) {                         // (this thread's own stores)
            const int64_t i = (int64_t)lod[p] * P + p;
            len = seg_start[i + 1] - seg_start[i];
            if (len < 0) len = 0;
        }
        long long x = len;
        for (int off = 1; off < 64; off <<= 1) {
            const long long y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
        }
        if (lane == 63) s_sum[wave] = x;
        __syncthreads();
        long long before = 0, all = 0;
        for (int w = 0; w < LOD_BLOCK / 64; ++w) {
            if (w < wave) before += s_sum[w];
            all += s_sum[w];
        }
        if (p < P) dst_start[p] = carry + before + x - len;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) {
        dst_start[P] = carry;
        record[0] = carry;
        record[1] = changed ? 1 : 0;
    }
}

struct LodArray { const float* src; float* dst; int width; int vec; unsigned chunk_end; };
struct LodArrays { LodArray a[5]; };

__global__ __launch_bounds__(LOD_BLOCK) void lod_gather_kernel(LodArrays arrays, int P, int L, int64_t R, int64_t n,
                                                               const int64_t* __restrict__ seg_start, const int8_t* __restrict__ lod,
                                                               const int64_t* __restrict__ dst_start) {
    const unsigned block = blockIdx.x;
    LodArray arr = arrays.a[0];
    unsigned first = 0;
#pragma unroll
    for (int k = 1; k < 5; ++k)
        if (block >= arrays.a[k - 1].chunk_end) { arr = arrays.a[k]; first = arrays.a[k - 1].chunk_end; }
    const int w = arr.width;
    const int64_t f0 = (int64_t)(block - first) * GATHER_CHUNK;
    const int64_t f1 = min(f0 + GATHER_CHUNK, n * (int64_t)w);
    if (f0 >= f1) return;
    const int tid = threadIdx.x;
    for (int p = lod_find_segment(dst_start, P, lod_row_of(f0, w)); p < P; ++p) {
        const int64_t ds = dst_start[p], de = dst_start[p + 1];
        if (ds * (int64_t)w >= f1) break;
        if (de <= ds) continue;
        const int level = lod[p];
        if (level < 0 || level >= L) continue;
        const int64_t sb = seg_start[(int64_t)level * P + p];
        if (sb < 0 || sb + (de - ds) > R) continue;       // (a table that does not hold the segment: nothing is read)
        const LodPiece piece = lod_piece(sb, ds, de, w, f0, f1);
        if (piece.len <= 0) continue;
        const int len = (int)piece.len;                   // <= GATHER_CHUNK
        if (arr.vec && ((piece.src | piece.dst | piece.len) & 3) == 0) {
            const float4* __restrict__ s = reinterpret_cast<const float4*>(arr.src + piece.src);
            float4* __restrict__ d = reinterpret_cast<float4*>(arr.dst + piece.dst);
            const int n4 = len >> 2;
            int i = tid;
            for (; i + 3 * LOD_BLOCK < n4; i += 4 * LOD_BLOCK) {
                const float4 v0 = s[i], v1 = s[i + LOD_BLOCK], v2 = s[i + 2 * LOD_BLOCK], v3 = s[i + 3 * LOD_BLOCK];
                d[i] = v0; d[i + LOD_BLOCK] = v1; d[i + 2 * LOD_BLOCK] = v2; d[i + 3 * LOD_BLOCK] = v3;
            }
            for (; i < n4; i += LOD_BLOCK) d[i] = s[i];
        } else {
            const float* __restrict__ s = arr.src + piece.src;
            float* __restrict__ d = arr.dst + piece.dst;
            int i = tid;
            for (; i + 3 * LOD_BLOCK < len; i += 4 * LOD_BLOCK) {
                const float v0 = s[i], v1 = s[i + LOD_BLOCK], v2 = s[i + 2 * LOD_BLOCK], v3 = s[i + 3 * LOD_BLOCK];
                d[i] = v0; d[i + LOD_BLOCK] = v1; d[i + 2 * LOD_BLOCK] = v2; d[i + 3 * LOD_BLOCK] = v3;
            }
            for (; i < len; i += LOD_BLOCK) d[i] = s[i];
        }
    }
}

}  // namespace gspl

extern "C" int gspl_lod_select(int P, int L, const float* camera_center, const float* transform, const float* box_min, const float* box_max,
                               const float* thresholds, const float* boxes3d, const float* world_to_camera, const float* K, int width,
                               int height, int visibility_filter, const int64_t* seg_start, const int8_t* prev_lod,
                               const uint8_t* prev_visible, float* distance, int8_t* lod, uint8_t* visible, int64_t* dst_start,
                               int64_t* record, void* stream) {
    using namespace gspl;
    if (P < 1 || P > LOD_MAX_PARTITIONS || L < 1 || L > LOD_MAX_LEVELS) return fail_arg("lod_select: P must be 1 .. 65536 and L 1 .. 127");
    if (!camera_center || !transform || !box_min || !box_max || !seg_start || !prev_lod || !prev_visible || !distance || !lod || !visible ||
        !dst_start || !record || ((L > 1) != (thresholds != nullptr)))
        return fail_arg("lod_select: NULL required pointer (thresholds is NULL iff L == 1)");
    if (visibility_filter && (!boxes3d || !world_to_camera || !K || width < 1 || height < 1))
        return fail_arg("lod_select: the visibility filter needs boxes3d, world_to_camera, K and the image size");
    hipLaunchKernelGGL(lod_select_kernel, dim3(1), dim3(LOD_BLOCK), 0, (hipStream_t)stream, P, L, camera_center, transform, box_min, box_max,
                       thresholds, boxes3d, world_to_camera, K, width, height, visibility_filter ? 1 : 0, seg_start, prev_lod, prev_visible,
                       distance, lod, visible, dst_start, record);
    return check_launch("lod_select");
}

extern "C" int gspl_lod_gather(int P, int L, int K, int64_t R, int64_t n, const int64_t* seg_start, const int8_t* lod,
                               const int64_t* dst_start, const float* means, const float* shs, const float* opacities, const float* scales,
                               const float* rotations, float* out_means, float* out_shs, float* out_opacities, float* out_scales,
                               float* out_rotations, void* stream) {
    using namespace gspl;
    if (P < 1 || P > LOD_MAX_PARTITIONS || L < 1 || L > LOD_MAX_LEVELS || K < 1 || K > GSPL_LOD_MAX_COEFFS || R < 0 || n < 0 || n > R)
        return fail_arg("lod_gather: P must be 1 .. 65536, L 1 .. 127, K 1 .. 64 and 0 <= n <= R");
    if (n == 0) return GSPL_OK;
    if (!seg_start || !lod || !dst_start || !means || !shs || !opacities || !scales || !rotations || !out_means || !out_shs ||
        !out_opacities || !out_scales || !out_rotations)
        return fail_arg("lod_gather: NULL required pointer");
    const float* src[5] = {means, shs, opacities, scales, rotations};
    float* dst[5] = {out_means, out_shs, out_opacities, out_scales, out_rotations};
    const int width[5] = {3, 3 * K, 1, 3, 4};
    LodArrays arrays;
    int64_t chunks = 0;
    for (int k = 0; k < 5; ++k) {
        chunks += (n * width[k] + GATHER_CHUNK - 1) / GATHER_CHUNK;
        if (chunks > 0x7fffffff) return fail_arg("lod_gather: more than 2^31 - 1 workgroups");
        arrays.a[k] = LodArray{src[k], dst[k], width[k], (aligned16(src[k]) && aligned16(dst[k])) ? 1 : 0, (unsigned)chunks};
    }
    hipLaunchKernelGGL(lod_gather_kernel, dim3((unsigned)chunks), dim3(LOD_BLOCK), 0, (hipStream_t)stream, arrays, P, L, R, n, seg_start, lod,
                       dst_start);
    return check_launch("lod_gather");
}

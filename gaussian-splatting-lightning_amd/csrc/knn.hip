// knn.hip — mean squared distance to the three nearest neighbours of every point (gfx950).
//
// Replaces `simple_knn._C.distCUDA2` (yzslab/simple-knn@44f76429, un-vendored), whose one call site sets the initial
// Gaussian scales from the SfM / random point cloud: internal/models/vanilla_gaussian.py:122-125
//     dist2 = clamp_min(distCUDA2(points), 1e-7);  scales = log(sqrt(dist2))
// Definition restated (the published simple-knn behaviour): for each point, the mean of the squared Euclidean
// distances (fp32) to its 3 nearest OTHER points (a coincident point is a neighbour at distance 0).
//
// Design: exact search on a uniform grid instead of the Morton-chunk search of the CUDA package.
//   1. bounds: min/max of the cloud (float atomics on order-preserving integer images)
//   2. cells:  cell edge h = cbrt(volume * TARGET / N), grid clamped to 256^3; per-point cell id, histogram
//   3. scan of the histogram (exclusive_scan_u32 of sort.hip), counting-sort scatter of the points into cell order
//   4. search: one lane per point walks the cube shells around its cell (Chebyshev radius r = 1, 2, ...), keeping the
//      three smallest d^2; after shell r every unvisited point is farther than r*h, so the search stops as soon as
//      the third-smallest d^2 <= (r*h)^2 — exact, and ~27 cells x TARGET points for a uniform cloud.
// One-shot at model initialisation (N = 1e5 .. 1e7), so the roofline is uninteresting; it takes ~1 ms per million points.
//
// knn_points (header section 19) is the general search on the same grid: a separate query set, any 1 <= K <= 32, distances AND
// indices, ordered by (d^2, index).  The grid is built over the reference cloud with a points-per-cell target that follows K; see
// knn_points_kernel for the walk, its stopping rule and where the K best live.
#include <cstring>
#include <cstdlib>
#include "gspl_device.h"
#include "gspl_host.h"
#include "gspl_sort.h"

namespace gspl {

static constexpr int KNN_MAX_DIM = 256;
static constexpr float KNN_TARGET = 6.f;       // points per cell aimed at by the 3-NN search
static constexpr int KNN_MAX_K = 32;
static constexpr int KNN_POINTS_BLOCK = 128;   // lanes (= queries) per workgroup of knn_points_kernel: K * 128 * 8 bytes of LDS

struct KnnGrid {
    float lo[3];
    float inv_h, h;
    int dim[3];
    float hi[3];      // the largest finite coordinate per axis (lo is the smallest): the box every finite point lies in
};

// order-preserving map float -> uint (so that unsigned atomicMin/Max order floats)
__device__ __forceinline__ unsigned f2ord(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

__global__ __launch_bounds__(256) void knn_bounds_init_kernel(unsigned* bounds) {
    if (threadIdx.x < 3) bounds[threadIdx.x] = 0xFFFFFFFFu;            // min images
    else if (threadIdx.x < 6) bounds[threadIdx.x] = 0u;                // max images
}

__global__ __launch_bounds__(256) void knn_bounds_kernel(int N, const float* __restrict__ pts, unsigned* __restrict__ bounds) {
    __shared__ unsigned s_min[3], s_max[3];
    if (threadIdx.x < 3) { s_min[threadIdx.x] = 0xFFFFFFFFu; s_max[threadIdx.x] = 0u; }
    __syncthreads();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = pts[i * 3 + a];
            if (v == v && fabsf(v) <= 3.0e38f) {       // NaN / inf coordinates do not stretch the grid
                const unsigned o = f2ord(v);
                atomicMin(&s_min[a], o);
                atomicMax(&s_max[a], o);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) { atomicMin(&bounds[threadIdx.x], s_min[threadIdx.x]); atomicMax(&bounds[3 + threadIdx.x], s_max[threadIdx.x]); }
}

// one thread: derive the grid from the bounds
__global__ void knn_grid_kernel(int N, const unsigned* __restrict__ bounds, KnnGrid* __restrict__ grid, unsigned long long capacity, float target) {
    float lo[3], hi[3], ext[3];
    for (int a = 0; a < 3; ++a) {
        const float mn = ord2f(bounds[a]), mx = ord2f(bounds[3 + a]);
        lo[a] = (mn <= mx) ? mn : 0.f;
        hi[a] = (mn <= mx) ? mx : 0.f;
        ext[a] = (mn <= mx) ? fmaxf(mx - mn, 0.f) : 0.f;
    }
    const float emax = fmaxf(ext[0], fmaxf(ext[1], ext[2]));
    float h;
    if (!(emax > 0.f)) {
        h = 1.f;                                   // all points coincide (or N <= 1)
    } else {
        // degenerate axes (a planar or linear cloud) count with a small thickness so that the cell edge stays sensible
        const float floor_e = emax * 1e-3f;
        const float vol = fmaxf(ext[0], floor_e) * fmaxf(ext[1], floor_e) * fmaxf(ext[2], floor_e);
        h = cbrtf(vol * target / (float)(N > 0 ? N : 1));
        h = fmaxf(h, emax / (float)KNN_MAX_DIM * 1.0001f);
    }
    int dim[3];
    for (int guard = 0; guard < 64; ++guard) {       // the cell arrays hold `capacity` cells: coarsen until the grid fits
        for (int a = 0; a < 3; ++a) dim[a] = min(KNN_MAX_DIM, max(1, (int)floorf(ext[a] / h) + 1));
        if ((unsigned long long)dim[0] * dim[1] * dim[2] <= capacity) break;
        h *= 1.26f;
    }
    grid->h = h;
    grid->inv_h = 1.f / h;
    for (int a = 0; a < 3; ++a) {
        grid->lo[a] = lo[a];
        grid->dim[a] = dim[a];
        grid->hi[a] = hi[a];
    }
}

__device__ __forceinline__ void cell_of(const KnnGrid& g, float x, float y, float z, int& cx, int& cy, int& cz) {
    // non-finite coordinates land in cell 0 (their distances are NaN/inf and never enter anybody's best three)
    const float fx = (x - g.lo[0]) * g.inv_h, fy = (y - g.lo[1]) * g.inv_h, fz = (z - g.lo[2]) * g.inv_h;
    cx = (fx == fx) ? min(g.dim[0] - 1, max(0, (int)fminf(fx, 1e6f))) : 0;
    cy = (fy == fy) ? min(g.dim[1] - 1, max(0, (int)fminf(fy, 1e6f))) : 0;
    cz = (fz == fz) ? min(g.dim[2] - 1, max(0, (int)fminf(fz, 1e6f))) : 0;
}

__global__ __launch_bounds__(256) void knn_count_kernel(int N, const float* __restrict__ pts, const KnnGrid* __restrict__ grid,
                                                        int32_t* __restrict__ cell_id, uint32_t* __restrict__ cell_count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const KnnGrid g = *grid;
    int cx, cy, cz;
    cell_of(g, pts[i * 3 + 0], pts[i * 3 + 1], pts[i * 3 + 2], cx, cy, cz);
    const int c = (cz * g.dim[1] + cy) * g.dim[0] + cx;
    cell_id[i] = c;
    atomicAdd(&cell_count[c], 1u);
}

// counting-sort scatter: cell_start is the exclusive scan of the counts; cursor (zeroed) hands out the slots of a cell
__global__ __launch_bounds__(256) void knn_scatter_kernel(int N, const float* __restrict__ pts, const int32_t* __restrict__ cell_id,
                                                          const uint32_t* __restrict__ cell_start, uint32_t* __restrict__ cursor,
                                                          float4* __restrict__ sorted) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int c = cell_id[i];
    const uint32_t slot = cell_start[c] + atomicAdd(&cursor[c], 1u);
    sorted[slot] = make_float4(pts[i * 3 + 0], pts[i * 3 + 1], pts[i * 3 + 2], __int_as_float(i));
}

__device__ __forceinline__ void push3(float d, float& b0, float& b1, float& b2) {
    if (d < b2) {
        if (d < b1) {
            b2 = b1;
            if (d < b0) { b1 = b0; b0 = d; } else { b1 = d; }
        } else {
            b2 = d;
        }
    }
}

__global__ __launch_bounds__(256) void knn_search_kernel(int N, const KnnGrid* __restrict__ grid, const uint32_t* __restrict__ cell_start,
                                                         const float4* __restrict__ sorted, float* __restrict__ out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;      // walk the points in cell order: neighbouring lanes, neighbouring cells
    if (s >= N) return;
    const KnnGrid g = *grid;
    const float4 p = sorted[s];
    const int self = __float_as_int(p.w);
    int cx, cy, cz;
    cell_of(g, p.x, p.y, p.z, cx, cy, cz);
    float b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;
    const int rmax = max(max(max(cx, g.dim[0] - 1 - cx), max(cy, g.dim[1] - 1 - cy)), max(cz, g.dim[2] - 1 - cz));
    auto visit = [&](int x, int y, int z) {
        const int c = (z * g.dim[1] + y) * g.dim[0] + x;
        const uint32_t lo = cell_start[c], hi = cell_start[c + 1];
        for (uint32_t k = lo; k < hi; ++k) {
            const float4 q = sorted[k];
            if (__float_as_int(q.w) == self) continue;
            const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
            push3(dx * dx + dy * dy + dz * dz, b0, b1, b2);
        }
    };
    for (int r = 0; r <= rmax; ++r) {
        // shell of Chebyshev radius r around (cx, cy, cz), clipped to the grid
        const int z0 = max(cz - r, 0), z1 = min(cz + r, g.dim[2] - 1);
        const int y0 = max(cy - r, 0), y1 = min(cy + r, g.dim[1] - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, g.dim[0] - 1);
        for (int z = z0; z <= z1; ++z) {
            const bool zface = (z == cz - r) || (z == cz + r);
            for (int y = y0; y <= y1; ++y) {
                const bool yface = (y == cy - r) || (y == cy + r);
                if (zface || yface) {
                    for (int x = x0; x <= x1; ++x) visit(x, y, z);
                } else {
                    if (cx - r >= 0) visit(cx - r, y, z);
                    if (r > 0 && cx + r <= g.dim[0] - 1) visit(cx + r, y, z);
                }
            }
        }
        // everything not visited yet is farther than r*h (the visited block extends at least r cells beyond the point's own)
        const float reach = (float)r * g.h * 0.99999f;       // margin for the rounding of the cell index
        if (b2 <= reach * reach) break;
    }
    // fewer than three other points (N <= 3): average what exists; a lone point gets 0
    float sum = 0.f;
    int n = 0;
    if (b0 < INFINITY) { sum += b0; ++n; }
    if (b1 < INFINITY) { sum += b1; ++n; }
    if (b2 < INFINITY) { sum += b2; ++n; }
    out[self] = (n == 3) ? sum / 3.f : (n > 0 ? sum / (float)n : 0.f);
}

// knn_points: the K nearest reference points of every query, as (d^2, index) ascending — among equal fp32 d^2 the lower index first.
//
// One lane per query.  A candidate is ONE 64-bit key, (bits of d^2) << 32 | index: d^2 >= 0, so the keys order as (d^2, index), a
// non-finite d^2 is refused before it becomes a key, and the all-ones key marks an empty slot.  Each lane keeps its K best keys as a
// sorted list in LDS, slot k of lane t at keys[k * BLOCK + t] (consecutive lanes, consecutive banks); an array indexed at run time
// in registers would live in scratch.  The largest kept key stays in a register, so a candidate costs one compare unless it enters.
// The set of cells a query visits depends only on the K-th key after each shell, never on the order of the points inside a cell
// (which the atomic cursor of the scatter leaves open): the result is the same bits on every run.
//
// The grid covers the box [lo, hi] of the reference cloud; a query may lie anywhere.  The walk starts from the cell of q', the query
// clamped into the box.  After shell r every unvisited point p lies more than r cell edges from q' along some axis, and because q'
// is the projection of q onto the box, |q_a - p_a| = |q_a - q'_a| + |q'_a - p_a| on every axis where q is outside: hence
// |q - p|^2 > |q - q'|^2 + (r h)^2.  The walk stops once the list is full and its K-th d^2 lies below that bound; `below` is kept
// strict by the margins (2e-4 cells for the rounding of the cell indices — up to 256 cells at fp32 — and 2e-6 relative for the
// rounding of the d^2 themselves), so no unvisited point can tie with the K-th on d^2 and win on its index.
__global__ __launch_bounds__(KNN_POINTS_BLOCK) void knn_points_kernel(int P1, const float* __restrict__ queries, int K, int cell_order,
                                                                      const KnnGrid* __restrict__ grid, const uint32_t* __restrict__ cell_start,
                                                                      const float4* __restrict__ sorted, float* __restrict__ dists,
                                                                      int64_t* __restrict__ idx) {
    extern __shared__ unsigned long long knn_keys[];
    constexpr unsigned long long EMPTY = ~0ull;
    const int t = threadIdx.x;
    const int s = blockIdx.x * KNN_POINTS_BLOCK + t;
    if (s >= P1) return;
    const int q = cell_order ? __float_as_int(sorted[s].w) : s;      // (self-query: P1 == P2 and `sorted` holds every index once)
    const float px = queries[(size_t)q * 3 + 0], py = queries[(size_t)q * 3 + 1], pz = queries[(size_t)q * 3 + 2];
    unsigned long long* keys = knn_keys + t;
    for (int k = 0; k < K; ++k) keys[k * KNN_POINTS_BLOCK] = EMPTY;
    unsigned long long worst = EMPTY;
    const KnnGrid g = *grid;
    const bool finite = fabsf(px) <= 3.0e38f && fabsf(py) <= 3.0e38f && fabsf(pz) <= 3.0e38f;      // (false for NaN)
    if (finite) {
        const float qx = fminf(fmaxf(px, g.lo[0]), g.hi[0]), qy = fminf(fmaxf(py, g.lo[1]), g.hi[1]), qz = fminf(fmaxf(pz, g.lo[2]), g.hi[2]);
        const float ox = px - qx, oy = py - qy, oz = pz - qz;
        const float off2 = ox * ox + oy * oy + oz * oz;
        int cx, cy, cz;
        cell_of(g, qx, qy, qz, cx, cy, cz);
        const int rmax = max(max(max(cx, g.dim[0] - 1 - cx), max(cy, g.dim[1] - 1 - cy)), max(cz, g.dim[2] - 1 - cz));
        auto visit = [&](int x, int y, int z) {
            const int c = (z * g.dim[1] + y) * g.dim[0] + x;
            const uint32_t lo = cell_start[c], hi = cell_start[c + 1];
            for (uint32_t n = lo; n < hi; ++n) {
                const float4 p = sorted[n];
                const float dx = p.x - px, dy = p.y - py, dz = p.z - pz;
                const float d2 = dx * dx + dy * dy + dz * dz;
                if (!(d2 <= 3.0e38f)) continue;                       // a non-finite reference point (or an overflow) is never a neighbour
                const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)__float_as_int(p.w);
                if (key < worst) {
                    int k = K - 1;
                    for (; k > 0; --k) {
                        const unsigned long long prev = keys[(k - 1) * KNN_POINTS_BLOCK];
                        if (prev < key) break;
                        keys[k * KNN_POINTS_BLOCK] = prev;
                    }
                    keys[k * KNN_POINTS_BLOCK] = key;
                    worst = keys[(K - 1) * KNN_POINTS_BLOCK];
                }
            }
        };
        for (int r = 0; r <= rmax; ++r) {
            const int z0 = max(cz - r, 0), z1 = min(cz + r, g.dim[2] - 1);
            const int y0 = max(cy - r, 0), y1 = min(cy + r, g.dim[1] - 1);
            const int x0 = max(cx - r, 0), x1 = min(cx + r, g.dim[0] - 1);
            for (int z = z0; z <= z1; ++z) {
                const bool zface = (z == cz - r) || (z == cz + r);
                for (int y = y0; y <= y1; ++y) {
                    const bool yface = (y == cy - r) || (y == cy + r);
                    if (zface || yface) {
                        for (int x = x0; x <= x1; ++x) visit(x, y, z);
                    } else {
                        if (cx - r >= 0) visit(cx - r, y, z);
                        if (r > 0 && cx + r <= g.dim[0] - 1) visit(cx + r, y, z);
                    }
                }
            }
            const float reach = fmaxf((float)r - 2e-4f, 0.f) * g.h;
            const float kth = __uint_as_float((unsigned)(worst >> 32));          // NaN while the list is not full: the test fails
            if (kth < (off2 + reach * reach) * 0.999998f) break;
        }
    }
    // fewer than K finite reference points: the rest of the row is zeros
    for (int k = 0; k < K; ++k) {
        const unsigned long long key = keys[k * KNN_POINTS_BLOCK];
        const bool have = key != EMPTY;
        dists[(size_t)q * K + k] = have ? __uint_as_float((unsigned)(key >> 32)) : 0.f;
        idx[(size_t)q * K + k] = have ? (int64_t)(unsigned)(key & 0xFFFFFFFFull) : 0;
    }
}

struct KnnWorkspace {
    size_t bounds_off, grid_off, cell_id_off, count_off, start_off, cursor_off, sorted_off, scan_tmp_off, scan_tmp_bytes, total;
};
static constexpr size_t KNN_MAX_CELLS = (size_t)KNN_MAX_DIM * KNN_MAX_DIM * KNN_MAX_DIM;

// cells actually allocated: the grid never has more than ~N / TARGET * 8 cells unless an axis hits the 256 clamp
static size_t knn_cell_capacity(int N) {
    const size_t want = (size_t)N * 4 + 4096;
    return want < KNN_MAX_CELLS ? want : KNN_MAX_CELLS;
}

static int plan_knn(int N, KnnWorkspace& w) {
    const size_t n = (size_t)(N > 0 ? N : 1), cells = knn_cell_capacity(N);
    const size_t scan_tmp = exclusive_scan_u32_workspace_bytes(cells + 1);
    Carve c;
    w.bounds_off = c.take(8 * 4);
    w.grid_off = c.take(sizeof(KnnGrid));
    w.cell_id_off = c.take(4 * n);
    w.count_off = c.take(4 * (cells + 1));
    w.start_off = c.take(4 * (cells + 1));
    w.cursor_off = c.take(4 * (cells + 1));
    w.sorted_off = c.take(16 * n);
    w.scan_tmp_bytes = scan_tmp;
    w.scan_tmp_off = c.take(scan_tmp);
    w.total = c.off;
    return GSPL_OK;
}

}  // namespace gspl

extern "C" size_t gspl_knn_workspace_bytes(int N) {
    gspl::KnnWorkspace w;
    if (N < 0 || gspl::plan_knn(N, w) != GSPL_OK) return 0;
    return w.total;
}

namespace gspl {
// bounds -> grid -> count -> scan -> scatter of `points` [N,3] into the workspace (N > 0); `target`: points per cell aimed at
static int knn_build_grid(int N, const float* points, float target, const KnnWorkspace& w, char* ws, hipStream_t s) {
    unsigned* bounds = (unsigned*)(ws + w.bounds_off);
    KnnGrid* grid = (KnnGrid*)(ws + w.grid_off);
    int32_t* cell_id = (int32_t*)(ws + w.cell_id_off);
    uint32_t* count = (uint32_t*)(ws + w.count_off);
    uint32_t* start = (uint32_t*)(ws + w.start_off);
    uint32_t* cursor = (uint32_t*)(ws + w.cursor_off);
    float4* sorted = (float4*)(ws + w.sorted_off);
    const size_t cells = knn_cell_capacity(N);
    const int grid_n = (N + 255) / 256;

    hipLaunchKernelGGL(knn_bounds_init_kernel, dim3(1), dim3(256), 0, s, bounds);
    hipLaunchKernelGGL(knn_bounds_kernel, dim3(std::min(grid_n, 1024)), dim3(256), 0, s, N, points, bounds);
    hipLaunchKernelGGL(knn_grid_kernel, dim3(1), dim3(1), 0, s, N, (const unsigned*)bounds, grid, (unsigned long long)cells, target);
    int rc = check_launch("knn_grid");
    if (rc != GSPL_OK) return rc;
    hipError_t e = hipMemsetAsync(count, 0, 4 * (cells + 1), s);
    if (e != hipSuccess) return check_hip(e, "knn: memset");
    e = hipMemsetAsync(cursor, 0, 4 * (cells + 1), s);
    if (e != hipSuccess) return check_hip(e, "knn: memset");
    hipLaunchKernelGGL(knn_count_kernel, dim3(grid_n), dim3(256), 0, s, N, points, (const KnnGrid*)grid, cell_id, count);
    rc = check_launch("knn_count");
    if (rc != GSPL_OK) return rc;
    rc = exclusive_scan_u32((const uint32_t*)count, start, cells + 1, ws + w.scan_tmp_off, s);
    if (rc != GSPL_OK) return rc;
    hipLaunchKernelGGL(knn_scatter_kernel, dim3(grid_n), dim3(256), 0, s, N, points, (const int32_t*)cell_id, (const uint32_t*)start, cursor, sorted);
    return check_launch("knn_scatter");
}
}  // namespace gspl

extern "C" int gspl_knn3_mean_dist2(int N, const float* points, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace gspl;
    if (N < 0) return fail_arg("knn3_mean_dist2: bad size");
    if (N == 0) return GSPL_OK;
    if (!points || !out || !workspace) return fail_arg("knn3_mean_dist2: NULL required pointer");
    KnnWorkspace w;
    int rc = plan_knn(N, w);
    if (rc != GSPL_OK) return rc;
    if (workspace_bytes < w.total) return fail_ws("knn3_mean_dist2");
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    rc = knn_build_grid(N, points, KNN_TARGET, w, ws, s);
    if (rc != GSPL_OK) return rc;
    hipLaunchKernelGGL(knn_search_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, (const KnnGrid*)(ws + w.grid_off),
                       (const uint32_t*)(ws + w.start_off), (const float4*)(ws + w.sorted_off), out);
    return check_launch("knn_search");
}

extern "C" size_t gspl_knn_points_workspace_bytes(int P2) { return gspl_knn_workspace_bytes(P2); }

extern "C" int gspl_knn_points(int P1, const float* p1, int P2, const float* p2, int K, float* dists, int64_t* idx,
                               void* workspace, size_t workspace_bytes, void* stream) {
    using namespace gspl;
    if (P1 < 0 || P2 < 0 || K < 1 || K > KNN_MAX_K) return fail_arg("knn_points: bad size (1 <= K <= 32)");
    if (P1 == 0) return GSPL_OK;
    if (!p1 || !dists || !idx) return fail_arg("knn_points: NULL required pointer");
    hipStream_t s = (hipStream_t)stream;
    if (P2 == 0) {      // nothing to find: the rows are the zero padding
        hipError_t e = hipMemsetAsync(dists, 0, sizeof(float) * (size_t)P1 * K, s);
        if (e == hipSuccess) e = hipMemsetAsync(idx, 0, sizeof(int64_t) * (size_t)P1 * K, s);
        return check_hip(e, "knn_points: memset");
    }
    if (!p2 || !workspace) return fail_arg("knn_points: NULL required pointer");
    KnnWorkspace w;
    int rc = plan_knn(P2, w);
    if (rc != GSPL_OK) return rc;
    if (workspace_bytes < w.total) return fail_ws("knn_points");
    char* ws = (char*)workspace;
    // the K nearest of a uniform cloud fill a ball of K points; with K / 2 points per cell its radius is ~0.8 cell edges, so most
    // queries stop after the 27 cells of the first shell
    rc = knn_build_grid(P2, p2, fmaxf(2.f, 0.5f * (float)K), w, ws, s);
    if (rc != GSPL_OK) return rc;
    // a self-query walks the queries in cell order: the lanes of a wave then walk neighbouring cells
    const bool self = (p1 == p2 && P1 == P2);
    const size_t lds = (size_t)K * KNN_POINTS_BLOCK * sizeof(unsigned long long);
    hipLaunchKernelGGL(knn_points_kernel, dim3((P1 + KNN_POINTS_BLOCK - 1) / KNN_POINTS_BLOCK), dim3(KNN_POINTS_BLOCK), lds, s, P1, p1, K, self ? 1 : 0,
                       (const KnnGrid*)(ws + w.grid_off), (const uint32_t*)(ws + w.start_off), (const float4*)(ws + w.sorted_off), dists, idx);
    return check_launch("knn_points");
}

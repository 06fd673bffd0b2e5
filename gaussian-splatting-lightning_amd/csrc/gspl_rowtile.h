// gspl_rowtile.h — streaming 16-byte accesses, and the flat copy of a workgroup's rows between global memory and LDS (device).
//
// A lane-per-row kernel whose rows are AoS (an SH coefficient row is 180 bytes) would read them as strided dwords, one cache line per
// lane and instruction.  Instead the workgroup copies its `rows` rows of `rs` floats, contiguous in global memory, as ONE flat run, 16
// bytes per lane, into LDS rows of ODD stride ls (lane r then reads row r without a bank conflict), and writes results back the same
// way in reverse.  Users: sh.hip (and its tile_adam, the Adam-applying tile_store), the tail of inria.hip, glossy.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace gspl {

// Nontemporal access of the i-th 16-byte piece behind `base` (16-byte aligned): for arrays streamed once per launch.
typedef float v4f __attribute__((ext_vector_type(4)));
template <class I>
__device__ __forceinline__ float4 load16_nt(const float* base, I i) {
    const v4f t = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(base) + i);
    return make_float4(t.x, t.y, t.z, t.w);
}
template <class I>
__device__ __forceinline__ void store16_nt(float* base, I i, const float4& q) {
    const v4f t = {q.x, q.y, q.z, q.w};
    __builtin_nontemporal_store(t, reinterpret_cast<v4f*>(base) + i);
}

// The row of flat element e, e / rs, from inv_rs = 1.f / (float)rs without an integer division.  e + 0.5 lies at least 0.5 / rs from
// the next multiple of rs and the product carries two roundings (relative error < 2^-23), so the result is exact while
// rows * rs <= 2^21; the tiles here are 256 rows of at most 75 floats.
__device__ __forceinline__ int tile_row(int e, float inv_rs) { return (int)(((float)e + 0.5f) * inv_rs); }

// `rows` rows of `rs` floats, contiguous behind g -> LDS rows of stride ls, by a workgroup of NT threads.  inv: 1.f / (float)rs, the
// caller's (a backward kernel loads and stores tiles of one width), with PART 1.f / (float)used.  vec_ok (g is 16-byte
// aligned): batches of U independent 16-byte loads per lane before any LDS write, U KiB per wave in flight (a load -> scatter -> load
// chain leaves the memory pipe idle most of the time: SQ_WAIT_ANY was 77 %); the floats behind the last whole piece one by one.
// PART, a compile-time choice (the run-time form costs the plain one registers): only the first `used` <= rs columns of a row are
// copied (used < rs: runs of `used` floats, one by one), and with `live` not NULL, one flag per row in LDS, only the rows that have
// one (a 16-byte piece is read when either of the two rows it can touch has one; used >= 3 there, so it touches no third).
template <int NT, int U, bool PART = false>
__device__ __forceinline__ void tile_load(const float* __restrict__ g, int rows, int rs, int ls, float inv, float* lds, bool vec_ok,
                                          int used = 0, const int* live = nullptr) {
    const int cols = PART ? used : rs;
    const int total = rows * cols;
    const int t = threadIdx.x;
    int done = 0;
    if (vec_ok && cols == rs) {
        const int n4 = total >> 2;
        auto wanted = [&](int e4) {
            if (e4 >= n4) return false;
            if constexpr (PART) {
                if (live) return (live[tile_row(e4 * 4, inv)] | live[tile_row(e4 * 4 + 3, inv)]) != 0;
            }
            return true;
        };
        for (int b4 = t; b4 < n4; b4 += NT * U) {
            float4 v[U];
            bool ok[U];      // (asked once per piece: with `live` the answer is two LDS reads)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e4 = b4 + u * NT;
                ok[u] = wanted(e4);
                v[u] = ok[u] ? load16_nt(g, e4) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e4 = b4 + u * NT;
                if (PART ? ok[u] : e4 < n4) {
                    const float vv[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int e = e4 * 4 + k;
                        const int row = tile_row(e, inv);
                        lds[row * ls + (e - row * rs)] = vv[k];
                    }
                }
            }
        }
        done = n4 << 2;
    }
    for (int e = done + t; e < total; e += NT) {
        const int row = tile_row(e, inv);
        if constexpr (PART) {
            if (live && !live[row]) continue;
            const int col = e - row * cols;
            lds[row * ls + col] = g[(int64_t)row * rs + col];
        } else {
            lds[row * ls + (e - row * rs)] = g[e];
        }
    }
}

// LDS rows of stride ls -> `rows` contiguous rows of rs floats behind g (inv_rs: 1.f / (float)rs; vec_ok: g is 16-byte aligned)
template <int NT>
__device__ __forceinline__ void tile_store(float* __restrict__ g, int rows, int rs, int ls, float inv_rs, const float* lds, bool vec_ok) {
    const int total = rows * rs;
    const int t = threadIdx.x;
    int done = 0;
    if (vec_ok) {
        const int n4 = total >> 2;
        for (int e4 = t; e4 < n4; e4 += NT) {
            float vv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = e4 * 4 + k;
                const int row = tile_row(e, inv_rs);
                vv[k] = lds[row * ls + (e - row * rs)];
            }
            store16_nt(g, e4, make_float4(vv[0], vv[1], vv[2], vv[3]));
        }
        done = n4 << 2;
    }
    for (int e = done + t; e < total; e += NT) {
        const int row = tile_row(e, inv_rs);
        g[e] = lds[row * ls + (e - row * rs)];
    }
}

}  // namespace gspl

// gspl_lod_index.h — the index arithmetic of the partition-LoD gather (lod.hip), host and device.  No HIP header: the host compiler
// alone builds it into a stand-alone program (tests/test_lod.py), the only place where offsets beyond 2^31 floats can be exercised.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GSPL_LOD_HD __host__ __device__
#else
#define GSPL_LOD_HD
#endif

namespace gspl {

// What one workgroup copies of one segment: `len` floats from float offset `src` of the table array to float offset `dst` of the
// destination array (len <= 0: nothing).
struct LodPiece { int64_t src, dst, len; };

// A segment of `dst_end - dst_begin` rows whose first row is row `src_begin` of the table and row `dst_begin` of the destination, in an
// array of `width` floats per row, cut to the workgroup's window [f0, f1) of destination FLOAT offsets.  Everything in 64 bits: at
// SH degree 3 (width 48) row 44 739 243 already starts beyond 2^31 floats.
GSPL_LOD_HD inline LodPiece lod_piece(int64_t src_begin, int64_t dst_begin, int64_t dst_end, int width, int64_t f0, int64_t f1) {
    const int64_t lo = dst_begin * (int64_t)width, hi = dst_end * (int64_t)width;
    const int64_t d0 = lo > f0 ? lo : f0, d1 = hi < f1 ? hi : f1;
    return LodPiece{src_begin * (int64_t)width + (d0 - lo), d0, d1 - d0};
}

// The first destination row a window starting at float offset f0 touches
GSPL_LOD_HD inline int64_t lod_row_of(int64_t f0, int width) { return f0 / (int64_t)width; }

// The last p in [0, P) with dst_start[p] <= row: the one segment that holds `row` when 0 <= row < dst_start[P] (empty segments share
// their start with the next one and are passed over).
GSPL_LOD_HD inline int lod_find_segment(const int64_t* dst_start, int P, int64_t row) {
    int lo = 0, hi = P - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (dst_start[mid] <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace gspl

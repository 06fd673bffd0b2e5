// gspl_host.h — host-side helpers shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "../../include/gspl_hip.h"

namespace gspl {

// thread-local last-error text, exposed through gspl_last_error()
void set_error(const char* where, const char* what);

inline int fail_arg(const char* msg) {
    set_error(msg, "invalid argument");
    return GSPL_ERR_INVALID_ARG;
}
inline int fail_ws(const char* msg) {
    set_error(msg, "workspace too small");
    return GSPL_ERR_WORKSPACE;
}
inline int check_launch(const char* where) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error(where, hipGetErrorString(e));
        return GSPL_ERR_LAUNCH;
    }
    return GSPL_OK;
}
inline int check_hip(hipError_t e, const char* where) {
    if (e != hipSuccess) {
        set_error(where, hipGetErrorString(e));
        return GSPL_ERR_LAUNCH;
    }
    return GSPL_OK;
}

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
// what the 16-byte accesses of the kernels ask of a base pointer (NULL passes: a caller for which NULL is no array says so itself)
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// One block carved into regions in the order they are taken, each starting on a 256-byte boundary; `off` ends as the block's size.
struct Carve {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off = up256(off + bytes); return o; }
};

// Run-time flags as template arguments: f is called with one std::bool_constant per flag, in the flags' order, and its result returned.
template <class F>
auto dispatch_bools(F&& f) { return f(); }
template <class F, class... Bs>
auto dispatch_bools(F&& f, bool b, Bs... rest) {
    auto bound = [&](auto c) { return dispatch_bools([&](auto... cs) { return f(c, cs...); }, rest...); };
    return b ? bound(std::true_type{}) : bound(std::false_type{});
}

// A run-time int as a template argument: f(std::integral_constant<int, V>) for the V of the list that equals `value`, and its result.
// A value outside the list is the call site's choice: with `otherwise` given, f is not called and `otherwise` returned; without, the
// LAST V of the list takes every other value (the caller has refused them).
template <int V0, int... Vs, class F, class R>
R dispatch_int(int value, F&& f, R otherwise) {
    if (value == V0) return f(std::integral_constant<int, V0>{});
    if constexpr (sizeof...(Vs) == 0) return otherwise;
    else return dispatch_int<Vs...>(value, f, otherwise);
}
template <int V0, int... Vs, class F>
auto dispatch_int(int value, F&& f) {
    if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V0>{});
    else return value == V0 ? f(std::integral_constant<int, V0>{}) : dispatch_int<Vs...>(value, f);
}

// A kernel templated on the compositing mode: f(MODE) gets it as a std::integral_constant (the caller has refused every other mode;
// gspl_composite.h has dispatch_composite for the <D, MODE, CHW> families).
template <class F>
auto dispatch_mode(int mode, F&& f) {
    if (mode == GSPL_MODE_GSPLAT) return f(std::integral_constant<int, GSPL_MODE_GSPLAT>{});
    return f(std::integral_constant<int, GSPL_MODE_INRIA>{});
}

// The pinned host words a binning scan stores the frame's list length into: one block of four per host thread, kept for the process.
// The calls that use it read their words before they return.  NULL (HIP's error cleared) when it cannot be allocated.
inline int64_t* pinned_words() {
    static thread_local int64_t* p = nullptr;
    if (!p) {
        void* q = nullptr;
        if (hipHostMalloc(&q, 4 * sizeof(int64_t), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        p = (int64_t*)q;
    }
    return p;
}

}  // namespace gspl

// ---- argument groups of the internal (non-ABI) interfaces ---------------------------------------------------------------------------
// Plain aggregates: an extern "C" entry fills them once, after its argument checks, and passes them down; the kernels keep their flat
// parameter lists and each launch site unpacks.  (A group exists where the same arguments cross three or more internal boundaries.)
namespace gspl {
struct TileGrid {      // the tiles the lists are cut on
    int size, w, h;
    int n() const { return w * h; }
};
inline TileGrid tile_grid16(int width, int height) { return TileGrid{16, (width + 15) / 16, (height + 15) / 16}; }
// what the binning reads of the projected splats (conics and opacities go together: both or neither) ...
struct BinSplats { int N, mode; const float* means2d; const int32_t* radii; const float* depths; const float* conics; const float* opacities; };
// ... and the depth order its count half leaves for its emission half: order [N], cum [N + 1], big_list [N], spans [GSPL_BIN_SPAN_BYTES * N]
struct BinOrder { int32_t* order; int64_t* cum; int32_t* big_list; void* spans; };

// SH coefficients as the colour kernels read them: the DC row and the rest, each with its float stride per splat.  One [N, n_coeffs, 3]
// array (rest == NULL) or the model's two arrays ([N, 1, 3] and [N, n_coeffs - 1, 3]); ShGrads: the matching gradients (or, with Adam
// in the backward, the parameters themselves)
struct ShCoeffs { const float* dc; int dc_stride; const float* rest; int rest_stride; };
struct ShGrads { float* dc; float* rest; };
inline ShCoeffs sh_coeffs(const float* shs, const float* shs_rest, int n_coeffs) {
    const int stride = 3 * n_coeffs;
    return shs_rest ? ShCoeffs{shs, 3, shs_rest, stride - 3} : ShCoeffs{shs, stride, shs + 3, stride};
}
inline ShGrads sh_grads(float* v_shs, float* v_shs_rest) { return v_shs_rest ? ShGrads{v_shs, v_shs_rest} : ShGrads{v_shs, v_shs + 3}; }
// How the SH backward kernels (sh.hip, and the one-launch tail of inria.hip) stage a splat's coefficient-gradient row in LDS:
//   merged  : tile rows are the full [K,3] rows starting at dc (row stride rs = dc_stride), dc at col 0, rest at col 3
//   separate: tile rows are the `rest` rows (row stride rs = rest_stride); dc is written per lane
struct ShTile {
    int rs;       // global row stride (floats)
    int ls;       // LDS row stride (odd)
    int merged;   // 1: dc inside the tile at col 0, rest at col 3
};
// The layout is decided on the OUTPUT arrays (they have the strides of the inputs); false: the row stride is too small for n_coeffs.
inline bool sh_grad_tile(const ShGrads& out, int dc_stride, int rest_stride, int n_coeffs, ShTile& tile) {
    tile.merged = (n_coeffs > 1 && out.rest == out.dc + 3 && dc_stride == rest_stride) ? 1 : 0;
    tile.rs = tile.merged ? dc_stride : rest_stride;
    if (n_coeffs > 1 && tile.rs < 3 * (n_coeffs - 1) + (tile.merged ? 3 : 0)) return false;
    if (n_coeffs <= 1) tile.rs = 1;
    tile.ls = tile.rs | 1;
    return true;
}

// the Inria rasterizer's camera ...
struct InriaCamera {
    const float* viewmatrix; const float* projmatrix; const float* campos;
    int width, height;
    float tanfovx, tanfovy, scale_modifier;
};
// ... its per-splat parameters (cov3d: the caller's precomputed covariances in the forward, the forward's own in the backward) ...
struct InriaParams {
    const float* means; const float* scales; const float* quats; const float* cov3d;
    const float* shs; const float* shs_rest;
    int degree, n_coeffs;
};
// ... and the per-splat gradients its compositing backward leaves: three columns of the packed rows x y | a b c | opacity | colour
// channels (stride 9, or 10 with 1 / z), or three dense arrays (stride 0, no opacity column)
struct SplatGradRows {
    const float* xy; const float* conic; const float* colour; const float* opacity; int stride;
    static SplatGradRows packed(const float* base, int stride) { return SplatGradRows{base, base + 2, base + 6, base + 5, stride}; }
};
// the gradients of the Inria parameters (with Adam in the backward: the parameters themselves, updated in place; means is then scratch [N,3])
struct InriaGrads {
    float* means; float* scales; float* quats; float* cov3d_precomp; float* shs; float* shs_rest; float* colors_precomp;
    float* means2d_ndc; float* opacities;
};
}  // namespace gspl

// internal launchers shared between translation units (sh.hip -> inria.hip)
namespace gspl {
int sh_fwd_launch(int N, int C, int degree, const float* dirs, const float* origin, ShCoeffs sh,
                  const uint8_t* mask, const int32_t* mask32, int flags,
                  float* colors, uint8_t* clamped, void* stream, float* jac /* nullable [N,9]: d colour / d unit direction */);
// Adam applied inside the per-Gaussian backward kernels (gspl_rasterize_inria_bwd_adam): moments + hyper-parameters of one parameter
typedef gspl_bwd_adam_tensor ShAdamTargetHost;
struct ShAdamHost { ShAdamTargetHost dc, rest; };
int sh_bwd_launch(int N, int C, int degree, int n_coeffs, const float* dirs, const float* origin, ShCoeffs sh,
                  const uint8_t* mask, const int32_t* mask32, int flags, const uint8_t* clamped,
                  const float* v_colors, int vc_stride, ShGrads v_sh, float* v_dirs, void* stream,
                  const float* jac /* nullable: the forward's Jacobian; v_dirs then needs no coefficient read */,
                  const ShAdamHost* adam /* nullable; not NULL: v_sh holds the PARAMETERS, updated in place, no gradient is written */,
                  bool prezeroed = false /* v_sh and v_dirs are cleared already: only rows with a non-zero colour gradient are written (one camera) */);
// A table that one kernel clears on behalf of a LATER kernel of the same stream (the tables of a prepared sort): the ~5 us
// radix_zero launch in front of that kernel goes away (profiles/r09_sequence.txt has the two of a frame).  16-byte units.
struct ZeroJob { uint4* p = nullptr; uint32_t n16 = 0; };
// binning.hip -> fused.hip: gspl_bin_count whose scan stores `ticket` into host_counts[2] after the two numbers.
// depth_header_zeroed: the caller's earlier kernel ran bin_depth_header()'s job.  `then_zero`: the last scan kernel runs this job
// (bin_tile_header(): the tables of the emission that follows).
int bin_count_ticket(const BinSplats& in, TileGrid grid, const BinOrder& ord, int64_t* host_counts,
                     void* workspace, size_t workspace_bytes, void* stream, unsigned long long ticket,
                     bool depth_header_zeroed = false, ZeroJob then_zero = ZeroJob());
int bin_depth_header(int N, int n_tiles, void* count_workspace, ZeroJob& job);                       // what bin_count would clear first
int bin_tile_header(int N, int64_t capacity, int n_tiles, void* workspace, ZeroJob& job);            // what gspl_bin_emit would clear first
int bin_emit_impl(const BinSplats& in, const BinOrder& ord, TileGrid grid, int64_t capacity, void* workspace, size_t workspace_bytes, void* stream,
                  bool tile_header_zeroed);
// The tile lists of a frame whose list length the host has read (count done, nothing emitted, or emitted into too little room): refuses
// more than 2^30-1 entries, then asks `alloc` for GSPL_BUF_LISTS_WORK, emits, asks for GSPL_BUF_LISTS and sorts, in that order.  No
// entries: *flatten_ids = NULL and `offsets` is filled with zeros.  `who` names the caller in the error texts.
int bin_lists_known(const BinSplats& in, const BinOrder& ord, TileGrid grid, int64_t n_isects, gspl_alloc_fn alloc, void* alloc_ctx,
                    int32_t** flatten_ids, int32_t* offsets, void* stream, const char* who);
// the density controller's statistics (gspl_densify_stats) applied by the preprocess backward itself; accum == NULL: not asked for
struct BwdStats { float* accum = nullptr; float* denom = nullptr; float* max_radii = nullptr; };
// inria.hip -> fused.hip: the geometry phase and the preprocess backward with the model's RAW parameters (GSPL_INRIA_RAW_PARAMS)
int inria_geometry_launch(int N, const InriaParams& p, const InriaCamera& cam, int tile_size,
                          int32_t* radii, float* means2d, float* depths, float* conics, float* cov3d,
                          const float* raw_opacities /* the caller's opacities, raw or not; read with either bit of `ext` */, float* opacities_out,
                          hipStream_t s, ZeroJob zero = ZeroJob() /* cleared by the same kernel, for the binning that follows */,
                          int ext = 0 /* GSPL_INRIA_RAW_PARAMS and / or GSPL_INRIA_ANTIALIAS: the one place that says RAW */);
// [N,4] rows colour | 1 / z for the inverse-depth channel of the fused call (GSPL_INRIA_INVDEPTH); colors4 16-byte aligned
int inria_invdepth_rows_launch(int N, const int32_t* radii, const float* colors3, const float* depths, float* colors4, hipStream_t s);
int inria_preprocess_bwd_impl(int N, const InriaParams& p, const InriaCamera& cam,
                              const int32_t* radii, const uint8_t* clamped, const SplatGradRows& rows, const InriaGrads& v, const float* sh_jac,
                              const float* opac_act /* read with RAW (the activated opacities) or ANTIALIAS (the caller's) in `ext` */, void* stream,
                              const gspl_bwd_adam_plan* adam = nullptr /* not NULL: v.shs / v.shs_rest / v.scales / v.quats / v.opacities are
                              the PARAMETERS (as means, scales, quats are), updated in place; v.means is scratch [N,3] */,
                              BwdStats stats = BwdStats(),
                              int ext = 0 /* GSPL_INRIA_RAW_PARAMS / GSPL_INRIA_ANTIALIAS / GSPL_INRIA_INVDEPTH: see inria.hip */,
                              uint8_t* grad_rows = nullptr /* [N], not NULL: every array of `v` is CLEARED already; rows whose packed gradient is
                              all zero are left alone, and grad_rows says which rows were written (inria.hip, PREZEROED) */);
}  // namespace gspl

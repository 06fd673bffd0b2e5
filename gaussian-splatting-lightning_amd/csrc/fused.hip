// fused.hip — ONE C-ABI call per direction for the Inria rasterizer (`gspl_rasterize_inria_fwd/bwd`).
//
// Replaces the call `diff_gaussian_rasterization.GaussianRasterizer.forward/backward` makes into its native library
// (reference call site: internal/renderers/vanilla_renderer.py:62-120; SURVEY.md §8b "fused gs_rasterize_vanilla_fwd/bwd,
// Inria argument list").  The stage entry points of this library (preprocess, binning, compositing) are orchestrated
// here, on the host side of the C boundary, instead of from Python: seven ctypes calls, two dozen torch allocations and
// their bookkeeping per forward become one call and three allocation call-backs — the Inria library's own pattern (its
// `resizeFunctional` lambdas grow three torch byte tensors: geometry, binning, image state).
//
// Nothing here launches kernels of its own; ownership stays with the caller: every buffer comes from `alloc(ctx, tag, bytes)`
// (torch's caching allocator on the Python side), nothing is hipMalloc'ed, the only persistent host resource is a small
// pinned word per thread for the one read-back of the frame (the list length that sizes the tile sort).
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <utility>
#include <vector>
#include "gspl_composite.h"
#include "gspl_sort.h"

namespace gspl {

// per-splat intermediates of one frame, carved out of ONE allocation (tag GSPL_BUF_GEOMETRY)
struct GeomLayout {
    size_t radii, means2d, depths, conics, colors, clamped, cov3d, sh_jac, order, cum, big_list, spans, opac, colors4, total;
};
// invdepth (GSPL_INRIA_INVDEPTH): one more region, the [N,4] rows compositing reads (colour | 1 / z)
static GeomLayout geom_layout(size_t n, bool invdepth = false) {
    GeomLayout g;
    Carve c;
    g.means2d = c.take(8 * n); g.depths = c.take(4 * n); g.conics = c.take(12 * n); g.colors = c.take(12 * n);
    g.clamped = c.take(3 * n); g.cov3d = c.take(24 * n); g.sh_jac = c.take(36 * n);
    g.order = c.take(4 * n); g.cum = c.take(8 * (n + 1)); g.big_list = c.take(4 * n); g.spans = c.take((size_t)GSPL_BIN_SPAN_BYTES * n);
    g.opac = c.take(4 * n);
    g.colors4 = invdepth ? c.take(16 * n) : 0;
    g.radii = 0;       // radii are an OUTPUT tensor of the call, not part of the block
    g.total = c.off;
    return g;
}
struct ImageLayout { size_t alphas, final_Ts, last_ids, offsets, total; };
static ImageLayout image_layout(size_t pixels, size_t tiles) {
    ImageLayout m;
    Carve c;
    m.alphas = c.take(4 * pixels); m.final_Ts = c.take(4 * pixels); m.last_ids = c.take(4 * pixels); m.offsets = c.take(4 * (tiles + 1));
    m.total = c.off;
    return m;
}

// The host's wait for the frame's one number (the list length): it POLLS the pinned word the scan kernel stores its ticket into.
// An event for it — hipEventRecord between the scan and the emission kernels — costs the stream a ~6 us bubble every frame.
// Bounded: every ~65 k polls the stream is queried; a stream that has drained (or failed) without the ticket arriving ends the wait.
static bool wait_for_ticket(const int64_t* host, unsigned long long ticket, hipStream_t s) {
    const volatile unsigned long long* flag = (const volatile unsigned long long*)(host + 2);
    for (unsigned spins = 1;; ++spins) {
        if (__atomic_load_n((const unsigned long long*)flag, __ATOMIC_ACQUIRE) == ticket) return true;
        __builtin_ia32_pause();
        if ((spins & 0xffffu) == 0u) {
            const hipError_t q = hipStreamQuery(s);
            if (q == hipSuccess) return __atomic_load_n((const unsigned long long*)flag, __ATOMIC_ACQUIRE) == ticket;
            if (q != hipErrorNotReady) { (void)hipGetLastError(); return false; }
        }
    }
}
// One lazily initialised T per device, for the process.  with(): f(the current device's T) under the table's lock, after init(T&) has
// once succeeded on that device; `fallback` for a device outside the table or an initialisation that failed (HIP's error cleared).
template <class T>
struct PerDevice {
    std::mutex mu;
    T slot[64] = {};
    bool ready[64] = {};
    template <class R, class Init, class F>
    R with(R fallback, Init&& init, F&& f) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return fallback;
        std::lock_guard<std::mutex> lk(mu);
        if (!ready[dev]) {
            if (!init(slot[dev])) { (void)hipGetLastError(); return fallback; }
            ready[dev] = true;
        }
        return f(slot[dev]);
    }
};

// Segmented backward, adaptive (gspl_composite.h): one word of pinned host memory per device that the backward kernels raise when a
// tile's walk is longer than a segment (written from the device, read by the host WITHOUT a synchronisation before a later forward —
// whenever it lands), and the number of frames the segmented form stays on after the word was last seen raised.  Process-wide:
// autograd runs the backward on a thread of its own.
// Per device: a ring of pinned host words the forward kernels store their verdicts into ((ticket << 1) | tail, about the PREVIOUS frame's
// backward), the view each slot's verdict is about, the verdicts per view, and the stream-level stickiness for views without one.
static constexpr unsigned SEG_RING = 16;
struct SegAdaptive {
    uint32_t* ring = nullptr;                 // pinned, SEG_RING words
    uint32_t slot_ticket[SEG_RING] = {};      // ticket a slot is waiting for (0: free)
    uintptr_t slot_view[SEG_RING] = {};       // ... and the view that verdict will be about
    uint32_t next = 1;
    uintptr_t prev_view = 0;                  // the view of the last forward (whose backward the next forward's kernel judges)
    int sticky = 0;
    std::unordered_map<uintptr_t, uint8_t> verdict;      // view -> 1 tail / 0 no tail
};
static PerDevice<SegAdaptive> g_seg;
// Called by the forward of a frame that may be segmented: collect the verdicts that have landed, decide for `view`, and hand out the ring
// slot + ticket this forward's kernel reports under.
static bool seg_decide(bool force, uintptr_t view, uint32_t** slot_out, uint32_t* ticket_out) {
    *slot_out = nullptr; *ticket_out = 0u;
    auto ring = [](SegAdaptive& a) {
        void* q = nullptr;
        if (hipHostMalloc(&q, SEG_RING * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) return false;
        a.ring = (uint32_t*)q;
        for (unsigned i = 0; i < SEG_RING; ++i) a.ring[i] = 0u;
        return true;
    };
    return g_seg.with(force, ring, [&](SegAdaptive& a) {
        for (unsigned i = 0; i < SEG_RING; ++i) {
            if (!a.slot_ticket[i]) continue;
            const uint32_t v = __atomic_load_n(a.ring + i, __ATOMIC_RELAXED);
            if ((v >> 1) != (a.slot_ticket[i] & 0x7fffffffu)) continue;      // not landed yet
            const bool tail = (v & 1u) != 0u;
            if (a.slot_view[i]) {
                if (a.verdict.size() > 65536) a.verdict.clear();
                a.verdict[a.slot_view[i]] = tail ? 1 : 0;
            }
            if (tail) a.sticky = 64;
            a.slot_ticket[i] = 0u;
        }
        bool on = force;
        const auto it = view ? a.verdict.find(view) : a.verdict.end();
        if (it != a.verdict.end()) on = on || it->second != 0;
        else on = on || a.sticky > 0;
        if (a.sticky > 0) --a.sticky;
        // this forward's kernel judges the backward of the previous forward's view
        const unsigned slot = a.next % SEG_RING;
        const uint32_t ticket = a.next & 0x7fffffffu;
        ++a.next; if ((a.next & 0x7fffffffu) == 0u) a.next = 1;
        a.slot_ticket[slot] = ticket;              // (an older verdict still waited for in this slot is given up: it never landed in 16 frames)
        a.slot_view[slot] = a.prev_view;
        a.prev_view = view;
        *slot_out = a.ring + slot; *ticket_out = ticket;
        return on;
    });
}
// the table the backward workgroups leave their walk lengths in (SEG_WALK_SLOTS rows of four words), one per device, zero at first
static PerDevice<uint32_t*> g_seg_walk;
static uint32_t* seg_walk_words() {
    auto zeroed = [](uint32_t*& words) {
        void* q = nullptr;
        const size_t bytes = (size_t)SEG_WALK_SLOTS * 4 * sizeof(uint32_t);
        if (hipMalloc(&q, bytes) != hipSuccess || hipMemset(q, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
            if (q) (void)hipFree(q);
            return false;
        }
        words = (uint32_t*)q;
        return true;
    };
    return g_seg_walk.with((uint32_t*)nullptr, zeroed, [](uint32_t* words) { return words; });
}

static unsigned long long next_ticket() {
    static thread_local unsigned long long t = 0ull;
    return ++t;
}

// three events per host thread (geometry done, colours done, count copied), created once
// (Measured, round 4: hipEventReleaseToDevice / hipEventDisableSystemFence on geo and col do not shorten the ~7 us the stream idles
// at an event record — it is the marker packet itself, not its fence.)
#ifndef GSPL_EVENT_FLAGS
#define GSPL_EVENT_FLAGS hipEventDisableTiming
#endif
struct FrameEvents { hipEvent_t geo = nullptr, col = nullptr, cnt = nullptr; bool ok = false; };
static FrameEvents& frame_events() {
    static thread_local FrameEvents ev;
    if (!ev.ok)
        ev.ok = hipEventCreateWithFlags(&ev.geo, GSPL_EVENT_FLAGS) == hipSuccess && hipEventCreateWithFlags(&ev.col, GSPL_EVENT_FLAGS) == hipSuccess &&
                hipEventCreateWithFlags(&ev.cnt, hipEventDisableTiming) == hipSuccess;
    return ev;
}

// A LOW-priority stream per device for the colour kernel (created once, never destroyed).  The colour kernel is a 70-90 us
// bandwidth stream that runs next to the latency-bound key pass and depth sort; at equal priority it takes half the machine
// from kernels that are on the critical path.  (torch.cuda.Stream cannot ask for a priority below the default.)
static PerDevice<hipStream_t> g_low_priority_streams;
extern "C" void* gspl_low_priority_stream(void) {
    auto create = [](hipStream_t& st) {
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (hipStreamCreateWithPriority(&st, hipStreamNonBlocking, least) == hipSuccess) return true;
        st = nullptr;
        return false;
    };
    return g_low_priority_streams.with((void*)nullptr, create, [](hipStream_t st) { return (void*)st; });
}

// Optional timing of the two compositing launches INSIDE the fused calls (bench.py's roofline: the launches cannot be bracketed
// from Python any more).  Events are recorded on the launch stream; durations are read after a synchronisation.
struct ProfSlot { std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; };
static int g_prof_period[2] = {0, 0};   // per direction; 0: off; k: every k-th launch is timed (an event pair costs ~6 us of stream idle time per side)
static unsigned g_prof_seen[2] = {0u, 0u};
static std::mutex g_prof_mu;
static ProfSlot g_prof[2];      // 0: composite forward, 1: composite backward
struct ProfScope {
    int which; hipStream_t s; hipEvent_t a = nullptr, b = nullptr;
    ProfScope(int w, hipStream_t st) : which(w), s(st) {
        if (g_prof_period[w] <= 0) return;
        if ((g_prof_seen[w]++ % (unsigned)g_prof_period[w]) != 0u) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
        (void)hipEventRecord(a, s);
    }
    ~ProfScope() {
        if (!a) return;
        (void)hipEventRecord(b, s);
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_prof[which].ev.emplace_back(a, b);
    }
};

}  // namespace gspl

extern "C" int gspl_profile_enable2(int period_fwd, int period_bwd) {
    std::lock_guard<std::mutex> lk(gspl::g_prof_mu);
    gspl::g_prof_period[0] = period_fwd > 0 ? period_fwd : 0;
    gspl::g_prof_period[1] = period_bwd > 0 ? period_bwd : 0;
    gspl::g_prof_seen[0] = gspl::g_prof_seen[1] = 0u;
    for (auto& slot : gspl::g_prof) {
        for (auto& e : slot.ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
        slot.ev.clear();
    }
    return GSPL_OK;
}

extern "C" int gspl_profile_enable(int period) { return gspl_profile_enable2(period, period); }

// which: 0 = composite forward, 1 = composite backward launches of the fused calls since gspl_profile_enable(1).
// Synchronises with the recorded events; returns the number of launches and their total duration.
extern "C" int gspl_profile_read(int which, int* count, float* total_ms) {
    using namespace gspl;
    if (which < 0 || which > 1 || !count || !total_ms) return fail_arg("profile_read: bad argument");
    std::lock_guard<std::mutex> lk(g_prof_mu);
    float tot = 0.f;
    for (auto& e : g_prof[which].ev) {
        float ms = 0.f;
        if (hipEventSynchronize(e.second) != hipSuccess || hipEventElapsedTime(&ms, e.first, e.second) != hipSuccess) return check_hip(hipGetLastError(), "profile_read");
        tot += ms;
    }
    *count = (int)g_prof[which].ev.size();
    *total_ms = tot;
    return GSPL_OK;
}

extern "C" size_t gspl_rasterize_inria_geometry_bytes(int N) { return gspl::geom_layout((size_t)(N > 0 ? N : 1)).total; }
extern "C" size_t gspl_rasterize_inria_image_bytes(int width, int height) {
    return gspl::image_layout((size_t)width * height, (size_t)((width + 15) / 16) * ((height + 15) / 16)).total;
}

namespace gspl {

static void carve_inria_state(gspl_inria_state* st, char* geom, const GeomLayout& g, char* img, const ImageLayout& im) {
    st->means2d = (float*)(geom + g.means2d); st->depths = (float*)(geom + g.depths); st->conics = (float*)(geom + g.conics);
    st->colors = (float*)(geom + g.colors); st->clamped = (uint8_t*)(geom + g.clamped); st->cov3d = (float*)(geom + g.cov3d);
    st->sh_jac = (float*)(geom + g.sh_jac);
    st->alphas = (float*)(img + im.alphas); st->final_Ts = (float*)(img + im.final_Ts); st->last_ids = (int32_t*)(img + im.last_ids);
    st->offsets = (int32_t*)(img + im.offsets);
}

// The wait for the scan's ticket as a scope, opened where the scan is enqueued: every way out of the scope has waited for the scan,
// because `host` is the thread's one block (pinned_words), free again after the call.
struct TicketWait {
    const int64_t* host; hipStream_t s;
    const unsigned long long ticket = next_ticket();
    bool waited = false, arrived = false;
    TicketWait(const int64_t* h, hipStream_t st) : host(h), s(st) {}
    TicketWait(const TicketWait&) = delete;
    bool wait() {      // whether the ticket arrived
        if (!waited) { arrived = wait_for_ticket(host, ticket, s); waited = true; }
        return arrived;
    }
    ~TicketWait() { (void)wait(); }
};
static int list_length_never_arrived(hipStream_t s) {
    const char* what = "rasterize_inria_fwd: the list length never arrived";
    return check_hip(hipStreamSynchronize(s), what) ? GSPL_ERR_LAUNCH : fail_arg(what);
}

// Segmented backward (gspl_composite.h): checkpoints + the frame's counters, sized by the list CAPACITY (known before the lists
// are: the guess, or the real length), from one allocation kept until the backward.  Off with GSPL_INRIA_NO_SEGMENTS, in the
// deterministic mode (its backward writes one row per list entry) and when the caller's allocator says no.
// (with or without checkpoints the forward kernel reduces the walk table the last backward left and reports its verdict)
struct SegPlan {
    bool adaptive = false, want = false;      // what seg_decide returned, with the ring slot + ticket this forward reports under
    uint32_t* verdict_slot = nullptr;
    uint32_t verdict_ticket = 0u;
    uint4* packed_zero = nullptr;             // the backward's packed rows, cleared by the forward's compositing kernel (GSPL_INRIA_WILL_BACKWARD, ABI 35)
    uint32_t packed_n16 = 0u;
    SegState seg = {};
    void ask_packed_rows(size_t row_bytes, gspl_alloc_fn alloc, void* alloc_ctx, gspl_inria_state* st) {
        const size_t bytes = (row_bytes + 15) & ~(size_t)15;
        packed_zero = (uint4*)alloc(alloc_ctx, GSPL_BUF_PACKED, bytes);
        if (packed_zero && bytes / 16 <= 0xffffffffull) { packed_n16 = (uint32_t)(bytes / 16); st->flags |= GSPL_INRIA_PACKED_READY; }
        else packed_zero = nullptr;
    }
    // what the compositing launch of lists with room for `cap` entries takes (NULL: nothing to do); asks for the checkpoint block
    const SegState* for_capacity(int64_t cap, bool invd, gspl_alloc_fn alloc, void* alloc_ctx, gspl_inria_state* st) {
        seg = SegState{};
        seg.zero_p = packed_zero; seg.zero_n16 = packed_n16;
        if (adaptive) { seg.walk = seg_walk_words(); seg.host_flag = verdict_slot; seg.ticket = verdict_ticket; }
        st->seg_ckpt = nullptr; st->seg_words = nullptr; st->seg_slots = 0u;
        if (!want || cap <= SEG) return (adaptive || packed_zero) ? &seg : nullptr;
        const uint32_t slots = (uint32_t)(cap >> SEG_LOG2) + 2u;
        const size_t words = 2 + (size_t)slots;
        const size_t head = up256(words * sizeof(uint32_t));
        // (with invd: one more float per checkpoint, the inverse-depth channel, after the float4s)
        char* blk = (char*)alloc(alloc_ctx, GSPL_BUF_CHECKPOINTS, head + (size_t)slots * 256 * (sizeof(float4) + (invd ? sizeof(float) : 0)));
        if (!blk) return (adaptive || packed_zero) ? &seg : nullptr;
        uint32_t* wds = (uint32_t*)blk;
        seg.words = wds; seg.slots = slots;      // (the item counter is cleared by the forward kernel itself)
        seg.ckpt = (float4*)(blk + head);
        seg.ckpt_x = invd ? (float*)(seg.ckpt + (size_t)slots * 256) : nullptr;
        st->seg_ckpt = seg.ckpt; st->seg_words = wds; st->seg_slots = slots;
        return &seg;
    }
};

// The colour chain of a frame, behind its geometry kernel: the SH kernel (and, with GSPL_INRIA_INVDEPTH, the [N,4] rows compositing reads),
// on the side stream when there is one.  *ev_col: what the caller's stream then waits for before compositing (NULL: same stream).
static int inria_colours_launch(int N, const InriaParams& p, const InriaCamera& cam, const float* colors_precomp, int32_t* radii, gspl_inria_state* st,
                                float* colors3, hipStream_t s, hipStream_t ss, hipEvent_t* ev_col) {
    FrameEvents& fe = frame_events();
    if (!fe.ok) return check_hip(hipGetLastError(), "rasterize_inria_fwd: event");
    const bool side = ss && ss != s;
    if (side) {
        (void)hipEventRecord(fe.geo, s);
        (void)hipStreamWaitEvent(ss, fe.geo, 0);
    }
    hipStream_t cs = side ? ss : s;
    int rc = gspl_inria_preprocess_fwd(N, p.degree, p.n_coeffs, p.means, p.scales, p.quats, p.cov3d, p.shs, p.shs_rest, colors_precomp, cam.viewmatrix,
                                       cam.projmatrix, cam.campos, cam.width, cam.height, 16, cam.tanfovx, cam.tanfovy, cam.scale_modifier, radii, st->means2d,
                                       st->depths, st->conics, colors3, st->clamped, st->cov3d, st->sh_jac, GSPL_INRIA_COLOURS, cs);
    if (rc == GSPL_OK && (st->flags & GSPL_INRIA_INVDEPTH)) rc = inria_invdepth_rows_launch(N, radii, colors3, st->depths, st->colors, cs);
    if (rc == GSPL_OK && side) { (void)hipEventRecord(fe.col, cs); *ev_col = fe.col; }
    return rc;
}

// the frame's compositing launch (n_isects < 0: the list length is on the device); colours are ready before compositing reads them
static int inria_composite_launch(int N, int D, const gspl_inria_state* st, const float* bg, int64_t n_isects, float* out_color,
                                  hipEvent_t ev_col, hipStream_t s, const SegState* sg) {
    if (ev_col) (void)hipStreamWaitEvent(s, ev_col, 0);
    ProfScope prof(0, s);
    return composite_fwd_impl(N, D, GSPL_MODE_INRIA, GSPL_LAYOUT_CHW, CompositeSplats{st->means2d, st->conics, st->colors, st->opacities, bg},
                              ImageSize{st->width, st->height}, tile_grid16(st->width, st->height), TileLists{st->offsets, st->flatten_ids, n_isects},
                              out_color, st->alphas, st->final_Ts, st->last_ids, nullptr, s, sg);
}

}  // namespace gspl

extern "C" int gspl_rasterize_inria_fwd(
    int N, int degree, int n_coeffs,
    const float* means3D, const float* scales, const float* rotations, const float* cov3D_precomp,
    const float* shs, const float* shs_rest, const float* colors_precomp, const float* opacities,
    const float* viewmatrix, const float* projmatrix, const float* campos, const float* bg,
    int width, int height, float tanfovx, float tanfovy, float scale_modifier,
    gspl_alloc_fn alloc, void* alloc_ctx, int64_t capacity_hint,
    float* out_color, int32_t* radii, gspl_inria_state* st, void* stream, void* side_stream) {
    using namespace gspl;
    const char* no_block = "rasterize_inria_fwd: allocation call-back returned NULL";
    if (N < 0 || width <= 0 || height <= 0 || !alloc || !st || !out_color) return fail_arg("rasterize_inria_fwd: bad argument");
    if (N > 0 && (!means3D || !opacities || !radii || !viewmatrix || !projmatrix || !campos)) return fail_arg("rasterize_inria_fwd: NULL required pointer");
    const TileGrid grid = tile_grid16(width, height);
    hipStream_t s = (hipStream_t)stream, ss = (hipStream_t)side_stream;
    const int flags = st->flags;
    if (flags & ~(GSPL_INRIA_RAW_PARAMS | GSPL_INRIA_NO_SEGMENTS | GSPL_INRIA_FORCE_SEGMENTS | GSPL_INRIA_WILL_BACKWARD | GSPL_INRIA_ANTIALIAS |
                  GSPL_INRIA_INVDEPTH)) return fail_arg("rasterize_inria_fwd: unknown state->flags (zero the struct before the call)");
    const bool raw = (flags & GSPL_INRIA_RAW_PARAMS) != 0;
    const bool aa = (flags & GSPL_INRIA_ANTIALIAS) != 0, invd = (flags & GSPL_INRIA_INVDEPTH) != 0;
    const int D = invd ? 4 : 3;                  // composited channels: colour (| inverse depth)
    const int prow = invd ? 10 : 9;              // the backward's packed row: x y | a b c | opacity | colour channels
    if (raw && (cov3D_precomp || (N > 0 && (!scales || !rotations)))) return fail_arg("rasterize_inria_fwd: raw parameters need scales and rotations");
    memset(st, 0, sizeof(*st));
    st->flags = flags;
    st->N = N; st->width = width; st->height = height;
    const size_t n = (size_t)(N > 0 ? N : 1);
    const GeomLayout g = geom_layout(n, invd);
    const ImageLayout im = image_layout((size_t)width * height, (size_t)grid.n());
    char* geom = (char*)alloc(alloc_ctx, GSPL_BUF_GEOMETRY, g.total);
    char* img = (char*)alloc(alloc_ctx, GSPL_BUF_IMAGE, im.total);
    if (!geom || !img) return fail_arg(no_block);
    carve_inria_state(st, geom, g, img, im);
    float* colors3 = st->colors;                  // where the colour kernel writes; with invd compositing reads the [N,4] rows
    if (invd) st->colors = (float*)(geom + g.colors4);
    const float* raw_opacities = (raw || aa) ? opacities : nullptr;      // (with aa: the caller's opacities, raw or activated)
    if (raw || aa) opacities = (float*)(geom + g.opac);          // from here on: what binning and compositing read
    st->opacities = const_cast<float*>(opacities);
    SegPlan plan;
    plan.adaptive = !(flags & GSPL_INRIA_NO_SEGMENTS) && gspl_get_deterministic() == 0;
    plan.want = plan.adaptive && seg_decide((flags & GSPL_INRIA_FORCE_SEGMENTS) != 0, (uintptr_t)viewmatrix, &plan.verdict_slot, &plan.verdict_ticket);
    if ((flags & GSPL_INRIA_WILL_BACKWARD) && N > 0) plan.ask_packed_rows((size_t)N * prow * sizeof(float), alloc, alloc_ctx, st);
    const BinSplats bins{N, GSPL_MODE_INRIA, st->means2d, radii, st->depths, st->conics, opacities};
    const BinOrder ord{(int32_t*)(geom + g.order), (int64_t*)(geom + g.cum), (int32_t*)(geom + g.big_list), geom + g.spans};
    if (N == 0) {
        const int rc = bin_lists_known(BinSplats{0, GSPL_MODE_INRIA}, BinOrder{}, grid, 0, alloc, alloc_ctx, &st->flatten_ids, st->offsets, s, "rasterize_inria_fwd");
        return rc != GSPL_OK ? rc : inria_composite_launch(N, D, st, bg, 0, out_color, nullptr, s, nullptr);
    }
    // every block whose size is known up front is asked for BEFORE the first launch: an allocation call-back costs the host
    // 5-10 us (it runs the caller's allocator), and between two launches that is a 6 us bubble on the device
    const size_t ws1_bytes = gspl_bin_workspace_bytes(N, 0);
    char* ws1 = (char*)alloc(alloc_ctx, GSPL_BUF_BINNING, ws1_bytes);
    if (!ws1) return fail_arg(no_block);
    const int64_t capacity = capacity_hint > 0 ? capacity_hint : 0;
    const size_t ws2_bytes = capacity ? gspl_bin_workspace_bytes(N, capacity) : 0;
    char* ws2 = capacity ? (char*)alloc(alloc_ctx, GSPL_BUF_LISTS_WORK, ws2_bytes) : nullptr;
    if (capacity && !ws2) return fail_arg(no_block);
    int64_t* host = pinned_words();
    if (!host) return fail_arg("rasterize_inria_fwd: no pinned host word");
    // geometry; then two independent chains: the colour (SH) kernel on the side stream, the count / depth-sort half of the
    // binning on the caller's stream; the host meanwhile waits for the one number that sizes the tile sort
    if (!viewmatrix || !projmatrix) return fail_arg("rasterize_inria_fwd: NULL required pointer");
    if (!cov3D_precomp && (!scales || !rotations)) return fail_arg("rasterize_inria_fwd: need scales+rotations or cov3D_precomp");
    // the geometry kernel clears the depth sort's tables, the scan kernel the tile sort's (when its workspace exists by then):
    // two launches fewer in front of the kernels that fill those tables
    ZeroJob zero_depth, zero_tile;
    int rc = bin_depth_header(N, grid.n(), ws1, zero_depth);
    if (rc == GSPL_OK && ws2) rc = bin_tile_header(N, capacity, grid.n(), ws2, zero_tile);
    if (rc != GSPL_OK) return rc;
    const InriaParams params{means3D, scales, rotations, cov3D_precomp, shs, shs_rest, degree, n_coeffs};
    const InriaCamera cam{viewmatrix, projmatrix, campos, width, height, tanfovx, tanfovy, scale_modifier};
    rc = inria_geometry_launch(N, params, cam, grid.size, radii, st->means2d, st->depths, st->conics, st->cov3d, raw_opacities, st->opacities, s, zero_depth,
                               flags & (GSPL_INRIA_RAW_PARAMS | GSPL_INRIA_ANTIALIAS));
    if (rc != GSPL_OK) return rc;
    hipEvent_t ev_col = nullptr;
    rc = inria_colours_launch(N, params, cam, colors_precomp, radii, st, colors3, s, ss, &ev_col);
    if (rc != GSPL_OK) return rc;
    TicketWait scan(host, s);      // the scan kernel stores the two numbers, then the ticket, into `host`
    rc = bin_count_ticket(bins, grid, ord, host, ws1, ws1_bytes, s, scan.ticket, true, zero_tile);
    if (rc != GSPL_OK) return rc;
    int64_t n_isects = 0;
    if (ws2) {
        // Speculative emission with the caller's guess of the list length.  The host does not wait for the real one: the sort reads it
        // on the device (the grid is sized by `capacity`), the compositing kernel finds the end of the last list in offsets[n_tiles].
        // The number is looked at AFTER everything is enqueued — by then the scan has long finished — and only a guess that turns out
        // too low costs a second round.
        rc = bin_emit_impl(bins, ord, grid, capacity, ws2, ws2_bytes, s, true);
        if (rc != GSPL_OK) return rc;
        st->flatten_ids = (int32_t*)alloc(alloc_ctx, GSPL_BUF_LISTS, 4 * (size_t)capacity);
        if (!st->flatten_ids) return fail_arg(no_block);
        const SegState* sg = plan.for_capacity(capacity, invd, alloc, alloc_ctx, st);
        rc = gspl_bin_sort_device_count(N, grid.w, grid.h, ord.cum + (N - 1), capacity, st->flatten_ids, st->offsets, ws2, ws2_bytes, s);
        if (rc != GSPL_OK) return rc;
        rc = inria_composite_launch(N, D, st, bg, -1, out_color, ev_col, s, sg);
        const bool arrived = scan.wait();
        n_isects = host[0];
        if (rc != GSPL_OK) return rc;
        if (!arrived) return list_length_never_arrived(s);
        if (n_isects <= capacity) { st->n_isects = n_isects; return GSPL_OK; }
        // too low a guess: the frame's lists are redone below with the real length
    } else {
        if (!scan.wait()) return list_length_never_arrived(s);
        n_isects = host[0];
    }
    rc = bin_lists_known(bins, ord, grid, n_isects, alloc, alloc_ctx, &st->flatten_ids, st->offsets, s, "rasterize_inria_fwd");
    if (rc != GSPL_OK) return rc;
    st->n_isects = n_isects;
    return inria_composite_launch(N, D, st, bg, n_isects, out_color, ev_col, s, plan.for_capacity(n_isects, invd, alloc, alloc_ctx, st));
}

namespace gspl {
// The sparse tail of the backward (gspl_rasterize_inria_bwd_sparse): the gradient arrays are cleared INSIDE the compositing backward's
// launch — a VALU-bound kernel that leaves HBM at 5 % — by a few extra workgroups at the front of its grid (composite_bwd.hip, FILL),
// and the per-splat kernels behind it then write only the rows that have a gradient.  Stream order is the only dependency: no second
// stream, no event in front of the compositing kernel or behind it.  One bounded grid over a table of the arrays, streaming stores: the
// compositing kernel keeps its wave slots and its L2.  How many workgroups (of 128 threads, the compositing kernel's): the fill has the
// ~300 us of the compositing backward to write 236 MB (1 M splats), and the faster it writes the more it delays that kernel's loads
// (profiles/tail_fill_in_grid.txt).  A frame without lists has no compositing launch: the fill is then a launch of its own.
#ifndef GSPL_FILL_BLOCKS
#define GSPL_FILL_BLOCKS 32
#endif
static int fill_blocks() {      // (GSPL_FILL_BLOCKS in the environment: A/B runs of what the fill costs the kernel it rides in; rounded up to a multiple of 8)
    static const int n = [] { const char* e = getenv("GSPL_FILL_BLOCKS"); const int v = e ? atoi(e) : 0; return ((v > 0 && v <= 65536 ? v : GSPL_FILL_BLOCKS) + 7) & ~7; }();
    return n;
}
__global__ __launch_bounds__(256) void zero_fill_kernel(FillJob job) { zero_fill_body<256>(job, blockIdx.x, gridDim.x); }
static FillJob grads_fill_job(int N, const InriaParams& p, const InriaGrads& v) {
    FillJob job;
    const uint64_t n = (uint64_t)N, sh_rows = (uint64_t)(p.n_coeffs > 0 ? p.n_coeffs : 0);
    job.add(v.means, 3 * n); job.add(v.means2d_ndc, 3 * n); job.add(v.opacities, n);
    job.add(v.scales, 3 * n); job.add(v.quats, 4 * n); job.add(v.cov3d_precomp, 6 * n); job.add(v.colors_precomp, 3 * n);
    if (v.shs_rest) { job.add(v.shs, 3 * n); job.add(v.shs_rest, 3 * (sh_rows > 0 ? sh_rows - 1 : 0) * n); }
    else job.add(v.shs, 3 * sh_rows * n);
    job.blocks = fill_blocks();
    return job;
}

// cam: width and height come from the state; p.cov3d: the forward's
static int rasterize_inria_bwd_impl(InriaParams p, const float* opacities, InriaCamera cam, const float* bg,
                                    const int32_t* radii, const gspl_inria_state* st, const float* v_out_color,
                                    float* packed /* [N, 9] scratch ([N, 10] with GSPL_INRIA_INVDEPTH) */, uint8_t* hit_flags,
                                    const InriaGrads& v, void* stream, const gspl_bwd_adam_plan* plan, uint8_t* grad_rows = nullptr) {
    if (!st || st->N < 0) return fail_arg("rasterize_inria_bwd: bad state");
    const int N = st->N;
    if (N == 0) return GSPL_OK;
    if (!packed || !v_out_color || !v.means || !v.means2d_ndc || !v.opacities) return fail_arg("rasterize_inria_bwd: NULL required pointer");
    cam.width = st->width; cam.height = st->height;
    p.cov3d = st->cov3d;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    const bool aa = (st->flags & GSPL_INRIA_ANTIALIAS) != 0, invd = (st->flags & GSPL_INRIA_INVDEPTH) != 0;
    const int D = invd ? 4 : 3, prow = invd ? 10 : 9;
    const float* caller_opacities = opacities;      // (aa: the backward of the compensation reads them, raw or activated)
    if (grad_rows && plan) return fail_arg("rasterize_inria_bwd: grad_rows and the optimizer inside the backward exclude each other");
    const FillJob fill = grad_rows ? grads_fill_job(N, p, v) : FillJob{};      // the sparse tail: the gradient arrays are cleared on the way
    if (!(st->flags & GSPL_INRIA_PACKED_READY)) {      // (else `packed` is the forward's GSPL_BUF_PACKED block, cleared by its compositing kernel)
        e = hipMemsetAsync(packed, 0, (size_t)N * prow * sizeof(float), s);      // x y | a b c | opacity | r g b (| 1/z)
        if (e != hipSuccess) return check_hip(e, "rasterize_inria_bwd: clear");
    }
    if (hit_flags) {
        e = hipMemsetAsync(hit_flags, 0, (size_t)N, s);
        if (e != hipSuccess) return check_hip(e, "rasterize_inria_bwd: clear");
    }
    const bool raw = (st->flags & GSPL_INRIA_RAW_PARAMS) != 0;
    if (raw) {
        if (!st->opacities || !v.scales || !v.quats) return fail_arg("rasterize_inria_bwd: raw parameters need the forward's state, v_scales and v_rotations");
        opacities = st->opacities;         // the activated values the forward composited with
    }
    if (aa) {
        if (!st->opacities) return fail_arg("rasterize_inria_bwd: anti-aliasing needs the forward's state");
        opacities = st->opacities;         // opacity * comp, what the forward composited with
    }
    if (st->n_isects > 0) {
        SegState seg = {};
        if (st->seg_ckpt && st->seg_words) {      // the forward left checkpoints: long walks are cut into segments (gspl_composite.h)
            seg.ckpt = (float4*)st->seg_ckpt;
            seg.words = st->seg_words; seg.slots = st->seg_slots;
            if (invd) seg.ckpt_x = (float*)(seg.ckpt + (size_t)seg.slots * 256);      // the inverse-depth channel's checkpoints
        }
        if (!(st->flags & GSPL_INRIA_NO_SEGMENTS) && gspl_get_deterministic() == 0) seg.walk = seg_walk_words();      // plain or segmented: the walk lengths are left for the next forward
        ProfScope prof(1, s);
        const int rc = composite_bwd_packed_impl(N, D, GSPL_MODE_INRIA, GSPL_LAYOUT_CHW, CompositeSplats{st->means2d, st->conics, st->colors, opacities, bg},
                                                 ImageSize{cam.width, cam.height}, tile_grid16(cam.width, cam.height),
                                                 TileLists{st->offsets, st->flatten_ids, st->n_isects}, st->final_Ts, st->last_ids, v_out_color, nullptr,
                                                 packed, prow, 0, hit_flags, s, &seg, grad_rows ? &fill : nullptr);
        if (rc != GSPL_OK) return rc;
    } else if (grad_rows) {      // no lists, no compositing launch to ride in
        hipLaunchKernelGGL(zero_fill_kernel, dim3(fill.blocks), dim3(256), 0, s, fill);
        const int rc = check_launch("rasterize_inria_bwd: clear the gradients");
        if (rc != GSPL_OK) return rc;
    }
    return inria_preprocess_bwd_impl(N, p, cam, radii, st->clamped, SplatGradRows::packed(packed, prow), v, st->sh_jac,
                                     aa ? caller_opacities : (raw ? st->opacities : nullptr), s, plan, BwdStats{st->stats_accum, st->stats_denom, st->stats_max_radii},
                                     st->flags & (GSPL_INRIA_RAW_PARAMS | GSPL_INRIA_ANTIALIAS | GSPL_INRIA_INVDEPTH), grad_rows);
}
}  // namespace gspl

extern "C" int gspl_rasterize_inria_bwd(
    int degree, int n_coeffs,
    const float* means3D, const float* scales, const float* rotations, const float* shs, const float* shs_rest, const float* opacities,
    const float* viewmatrix, const float* projmatrix, const float* campos, const float* bg,
    float tanfovx, float tanfovy, float scale_modifier,
    const int32_t* radii, const gspl_inria_state* st, const float* v_out_color,
    float* packed, uint8_t* hit_flags,
    float* v_means3D, float* v_means2D_ndc, float* v_shs, float* v_shs_rest, float* v_colors_precomp, float* v_opacities,
    float* v_scales, float* v_rotations, float* v_cov3D, void* stream) {
    using namespace gspl;
    return rasterize_inria_bwd_impl(InriaParams{means3D, scales, rotations, nullptr, shs, shs_rest, degree, n_coeffs}, opacities,
                                    InriaCamera{viewmatrix, projmatrix, campos, 0, 0, tanfovx, tanfovy, scale_modifier}, bg, radii, st, v_out_color, packed, hit_flags,
                                    InriaGrads{v_means3D, v_scales, v_rotations, v_cov3D, v_shs, v_shs_rest, v_colors_precomp, v_means2D_ndc, v_opacities}, stream, nullptr);
}

// The same backward for a saturated frame, in which most splats get no gradient: the gradient arrays are cleared inside the compositing
// backward and the per-splat kernels write only the rows that have one; grad_rows [N] says which.  Same values as
// gspl_rasterize_inria_bwd (a zero may differ in sign).
extern "C" int gspl_rasterize_inria_bwd_sparse(
    int degree, int n_coeffs,
    const float* means3D, const float* scales, const float* rotations, const float* shs, const float* shs_rest, const float* opacities,
    const float* viewmatrix, const float* projmatrix, const float* campos, const float* bg,
    float tanfovx, float tanfovy, float scale_modifier,
    const int32_t* radii, const gspl_inria_state* st, const float* v_out_color,
    float* packed, uint8_t* hit_flags,
    float* v_means3D, float* v_means2D_ndc, float* v_shs, float* v_shs_rest, float* v_colors_precomp, float* v_opacities,
    float* v_scales, float* v_rotations, float* v_cov3D, uint8_t* grad_rows, void* stream) {
    using namespace gspl;
    if (!grad_rows) return fail_arg("rasterize_inria_bwd_sparse: NULL grad_rows");
    return rasterize_inria_bwd_impl(InriaParams{means3D, scales, rotations, nullptr, shs, shs_rest, degree, n_coeffs}, opacities,
                                    InriaCamera{viewmatrix, projmatrix, campos, 0, 0, tanfovx, tanfovy, scale_modifier}, bg, radii, st, v_out_color, packed, hit_flags,
                                    InriaGrads{v_means3D, v_scales, v_rotations, v_cov3D, v_shs, v_shs_rest, v_colors_precomp, v_means2D_ndc, v_opacities}, stream, nullptr,
                                    grad_rows);
}

// The same backward with the optimizer INSIDE it: the per-Gaussian kernels at the end of the backward (SH backward,
// preprocess backward) apply the Adam update to the parameter rows they have just produced the gradient of, instead of writing
// 236 B of gradient per Gaussian for a separate optimizer launch to read back.  The parameters are updated IN PLACE; only the
// screen-space gradient (what the density controller reads, vanilla_density_controller.py:101-123) is written.
extern "C" int gspl_rasterize_inria_bwd_adam(
    int degree, int n_coeffs,
    float* means3D, float* scales, float* rotations, float* shs, float* shs_rest, float* opacities,
    const float* viewmatrix, const float* projmatrix, const float* campos, const float* bg,
    float tanfovx, float tanfovy, float scale_modifier,
    const int32_t* radii, const gspl_inria_state* st, const float* v_out_color,
    float* packed, uint8_t* hit_flags, float* scratch_means, float* v_means2D_ndc, const gspl_bwd_adam_plan* plan, void* stream) {
    using namespace gspl;
    if (!plan) return fail_arg("rasterize_inria_bwd_adam: NULL plan");
    if (!scales || !rotations || !shs || !opacities) return fail_arg("rasterize_inria_bwd_adam: needs scales, rotations, SH coefficients and opacities");
    if (st && (st->flags & (GSPL_INRIA_ANTIALIAS | GSPL_INRIA_INVDEPTH)))
        return fail_arg("rasterize_inria_bwd_adam: a frame rendered with GSPL_INRIA_ANTIALIAS or GSPL_INRIA_INVDEPTH takes gspl_rasterize_inria_bwd and a separate optimizer");
    return rasterize_inria_bwd_impl(InriaParams{means3D, scales, rotations, nullptr, shs, shs_rest, degree, n_coeffs}, opacities,
                                    InriaCamera{viewmatrix, projmatrix, campos, 0, 0, tanfovx, tanfovy, scale_modifier}, bg, radii, st, v_out_color, packed, hit_flags,
                                    InriaGrads{scratch_means, scales, rotations, nullptr, shs, shs_rest, nullptr, v_means2D_ndc, opacities}, stream, plan);
}

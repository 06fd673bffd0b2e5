"""Direct C-ABI call helpers for the GPU parity tests (tests only)."""
import numpy as np
import torch

from gspl_amd import _lib as L


def dev():
    return torch.device("cuda:0")


# Multi-process GPU tests run at most this many ranks on cuda:0.  Every rank holds the device, and so does the pytest process that
# started them; the hosts the suite runs on admit six processes with a GPU open, and eight ranks were stopped there.  The eight-way
# peer transport is exercised at the kernel level in one process (test_peer_exchange.py::test_eight_way_put_signal_wait_in_one_process).
MAX_RANKS_SHARING_A_GPU = 4


def t32(a, device=None):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32).contiguous().to(device or dev())


def hip_composite_fwd(mode, means2d, conics, colors, opac, bg, W, H, offsets, flat, layout=L.GSPL_LAYOUT_HWC, hits=None, tile=16):
    lib = L.lib()
    N, D = colors.shape
    tw, th = (W + tile - 1) // tile, (H + tile - 1) // tile
    shape = (H, W, D) if layout == L.GSPL_LAYOUT_HWC else (D, H, W)
    out = torch.empty(shape, dtype=torch.float32, device=means2d.device)
    alphas = torch.empty((H, W), dtype=torch.float32, device=means2d.device)
    final_T = torch.empty((H, W), dtype=torch.float32, device=means2d.device)
    last = torch.empty((H, W), dtype=torch.int32, device=means2d.device)
    n_isects = flat.shape[0]
    L.check(lib.gspl_composite_fwd(N, n_isects, D, mode, layout, L.ptr(means2d), L.ptr(conics), L.ptr(colors), L.ptr(opac),
                                   L.ptr(bg), W, H, tile, tw, th, L.ptr(offsets), L.ptr(flat) if n_isects else None,
                                   L.ptr(out), L.ptr(alphas), L.ptr(final_T), L.ptr(last), L.ptr(hits), L.stream()), "composite_fwd")
    return out, alphas, final_T, last


def hip_composite_bwd(mode, means2d, conics, colors, opac, bg, W, H, offsets, flat, final_T, last, v_out, v_alpha=None,
                      absgrad=False, layout=L.GSPL_LAYOUT_HWC, tile=16):
    lib = L.lib()
    N, D = colors.shape
    tw, th = (W + tile - 1) // tile, (H + tile - 1) // tile
    d = means2d.device
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=d)
    v_xy, v_con, v_col, v_op = z(N, 2), z(N, 3), z(N, D), z(N)
    v_abs = z(N, 2) if absgrad else None
    hit = torch.zeros(N, dtype=torch.uint8, device=d)
    L.check(lib.gspl_composite_bwd(N, flat.shape[0], D, mode, layout, L.ptr(means2d), L.ptr(conics), L.ptr(colors), L.ptr(opac),
                                   L.ptr(bg), W, H, tile, tw, th, L.ptr(offsets), L.ptr(flat), L.ptr(final_T), L.ptr(last),
                                   L.ptr(v_out), L.ptr(v_alpha), L.ptr(v_xy), L.ptr(v_abs), L.ptr(v_con), L.ptr(v_col),
                                   L.ptr(v_op), L.ptr(hit), L.stream()), "composite_bwd")
    return dict(v_means2d=v_xy, v_means2d_abs=v_abs, v_conics=v_con, v_colors=v_col, v_opacities=v_op, hit=hit)


# The density controllers' opacity reset (vanilla_density_controller.py, `_reset_opacities`; opacity_reset_value = 0.01): the stored
# logit becomes inverse_sigmoid(min(sigmoid(logit), value)), so every clamped splat renders at fp32 sigmoid(logit(0.01)) = 0.0099999988.
RESET_OPACITY = 0.009999998845160007


def reset_opacities(opac, value=0.01):
    """What the model's activated opacities are right after an opacity reset, in fp32 as the reference computes them: the inverse
    sigmoid log(x / (1 - x)) of min(o, value), then the model's sigmoid."""
    o = torch.as_tensor(opac, dtype=torch.float32)
    x = torch.minimum(o, torch.full_like(o, value))
    return torch.sigmoid(torch.log(x / (1 - x)))


EPS32 = 2.0 ** -24


def cov2d_condition(conics) -> np.ndarray:
    """lambda_max / lambda_min of every splat's 2D covariance (= of its conic), from the oracle's fp64 conics [N,3]."""
    c = np.asarray(conics, np.float64)
    tr, det = c[:, 0] + c[:, 2], c[:, 0] * c[:, 2] - c[:, 1] ** 2
    disc = np.sqrt(np.maximum(tr * tr / 4 - det, 0.0))
    lo = np.maximum(tr / 2 - disc, 1e-300)
    return np.where(det > 0, (tr / 2 + disc) / lo, 1.0)


def cov_chain_slack(ref, kappa, factor=200.0) -> np.ndarray:
    """Per-ELEMENT absolute slack for gradients that pass through conic -> cov2D -> cov3D (means, scales, rotations):
    factor * eps32 * kappa_row * max|ref_row|.  Why: dL/dcov2D = -conic G conic with G = dL/dconic; for an elongated splat G is
    dominated by the long axis (sum of sp dx^2 over hundreds of pixels) and conic by the short one, the two nearly annihilate, and
    what survives carries the rounding of the products: a RELATIVE error ~ eps32 * kappa(cov2D) in fp32, in this kernel and in any
    fp32 evaluation of the reference's formulation (diff_gaussian_rasterization and gsplat compute exactly this product in fp32).
    Measured on `synthetic.scene_surfaces` with the compositing gradients equal to 1e-6 (profiles/r07d_locked_rows_diag.txt):
    rows with kappa 400 ... 4100 are off by 60 ... 100 x eps32 x kappa of their own magnitude; factor 200 bounds that with a
    margin of two.  For kappa <= 8 (the bulk of a scene) the slack is below 1e-4 of the row: the plain tolerance decides."""
    ref = np.asarray(ref, np.float64)
    rowmax = np.abs(ref).reshape(len(ref), -1).max(axis=1)
    slack = factor * EPS32 * np.asarray(kappa, np.float64) * rowmax
    return slack.reshape((len(ref),) + (1,) * (ref.ndim - 1)) * np.ones_like(ref)


def cov_chain_bound(api, params, cam, H, W, mask, v_conics, radii, factor=8.0):
    """Running fp32 rounding bound of the gradients that pass through conic -> cov2D -> cov3D -> (means, scales, rotations), per
    ELEMENT, from fp64 quantities only (a first-order error analysis of the chain every implementation of the reference's
    formulation evaluates — diff_gaussian_rasterization and gsplat in fp32 too):

      1. dL/dcov2D = -conic G conic, written out on the cov2D entries (a, b, c):
             va = (-c c vA + b c vB - b b vC) / det^2,   vb = (2 b c vA - (a c + b b) vB + 2 a b vC) / det^2,   vc likewise
         (G = (vA, vB, vC) = dL/dconic, det = a c - b b).  For an elongated splat G is dominated by the long axis and conic by the
         short one: the three products are ~ kappa^2 times their sum.  Rounding error <= eps32 * Tx, Tx = sum of |products| / det^2.
      2. dL/dSigma_ij = sum_x vx dx/dSigma_ij (x in a, b, c; dx/dSigma_ij = T_ai T_bj) and dL/dtheta = sum_ij dL/dSigma_ij dSigma_ij/dtheta
         (theta = scales, rotations), dL/dmean = sum_x vx dx/dmean: sums of products of mixed sign again; what an error of stage 1 — and
         the rounding of these sums themselves — can amount to is the same chain run on absolute values:
             A_theta = sum_ij |dSigma_ij/dtheta| sum_x |dx/dSigma_ij| Tx,        A_mean = sum_x |dx/dmean| Tx.
      3. G itself is an fp32 sum over the splat's footprint: each of its entries carries factor * eps32 * sqrt(pixels) of its size
         (footprint_slack: what the compositing kernel's own gradients are held to), and an error of G goes through the same chain.
      bound = factor * eps32 * (1 + sqrt(pi) r) * A  (`factor`: the handful of roundings per product and stage, with a margin of two;
      r = the splat's radius in pixels).  Not tight — a first-order worst case — but it scales with what makes the chain
      ill-conditioned and vanishes (below 1e-4 of the row) for the round splats that make up the bulk of a scene.

    The Jacobians come from torch.autograd on the oracle's own stages (cov3d_from_scale_rot, ewa_cov2d), one unit cotangent each.
    api "vanilla": Inria conventions (near plane 0.2, clamped coordinates constant in the backward); "gsplat": near 0.01.
    v_conics [N,3] = the oracle's dL/dconic.  Returns {"means": [N,3], "scales": [N,3], "quats": [N,4]}."""
    import torch
    from oracle import gsplat_oracle as O
    m, s, q = [t.detach().double().clone().requires_grad_(True) for t in params[:3]]
    V = cam["world_to_camera"].double()
    pv = m @ V[:3, :3] + V[3, :3]
    front = pv[:, 2].detach() >= (0.2 if api == "vanilla" else 0.01)
    pv_safe = torch.where(front[:, None], pv, torch.ones_like(pv))
    sigma = O.cov3d_from_scale_rot(s, 1.0, q)
    sigma_leaf = sigma.detach().clone().requires_grad_(True)
    if api == "vanilla":
        fx, fy = W / (2.0 * cam["tanfovx"]), H / (2.0 * cam["tanfovy"])
        cov2d = O.ewa_cov2d(pv_safe, sigma_leaf, V[:3, :3].T, fx, fy, 1.3 * cam["tanfovx"], 1.3 * cam["tanfovy"], inria_clamp_grad=True)
    else:
        fx, fy = float(cam["fx"]), float(cam["fy"])
        cov2d = O.ewa_cov2d(pv_safe, sigma_leaf, V[:3, :3].T, fx, fy, 1.3 * (0.5 * W / fx), 1.3 * (0.5 * H / fy))
    a, b, c = cov2d[:, 0, 0] + 0.3, cov2d[:, 0, 1], cov2d[:, 1, 1] + 0.3
    an, bn, cn = (np.abs(t.detach().numpy()) for t in (a, b, c))
    vA, vB, vC = (np.abs(np.asarray(v_conics, np.float64)[:, k]) for k in range(3))
    det2 = np.maximum((a.detach().numpy() * c.detach().numpy() - b.detach().numpy() ** 2) ** 2, 1e-300)
    T = {"a": (cn * cn * vA + bn * cn * vB + bn * bn * vC) / det2,
         "b": (2 * bn * cn * vA + (an * cn + bn * bn) * vB + 2 * an * bn * vC) / det2,
         "c": (bn * bn * vA + an * bn * vB + an * an * vC) / det2}
    A_sigma, A_m = np.zeros((len(an), 3, 3)), np.zeros((len(an), 3))
    for x, key in ((a, "a"), (b, "b"), (c, "c")):
        g_sigma, g_m = torch.autograd.grad(x.sum(), [sigma_leaf, m], retain_graph=True)
        A_sigma += np.abs(g_sigma.numpy()) * T[key][:, None, None]
        A_m += np.abs(g_m.numpy()) * T[key][:, None]
    A_s, A_q = np.zeros((len(an), 3)), np.zeros((len(an), 4))
    for i in range(3):
        for j in range(3):
            g_s, g_q = torch.autograd.grad(sigma[:, i, j].sum(), [s, q], retain_graph=True)
            A_s += np.abs(g_s.numpy()) * A_sigma[:, i, j, None]
            A_q += np.abs(g_q.numpy()) * A_sigma[:, i, j, None]
    keep = (np.asarray(mask, bool) & front.numpy())[:, None]
    scale = (factor * EPS32 * (1.0 + np.sqrt(np.pi) * np.maximum(np.asarray(radii, np.float64), 1.0)))[:, None]
    return {n: scale * np.where(keep, A, 0.0) for n, A in (("means", A_m), ("scales", A_s), ("quats", A_q))}


def footprint_slack(ref, radii, factor=8.0) -> np.ndarray:
    """Per-element absolute slack for the compositing kernel's per-splat sums: factor * eps32 * sqrt(pixels of the splat's footprint) *
    max|ref_row|.  A per-splat gradient is an fp32 sum of one signed term per covered pixel; over n terms of mixed sign it carries
    ~ eps32 sqrt(n) of the terms' magnitude, and for the moments of a long splat (sum of sp dx, sp dx^2 over a footprint hundreds of
    pixels wide) that magnitude is several times the result.  Radius 10 px: 1e-5 of the row — the plain 1e-4 decides; radius 600 px (the
    longest needles of `scene_surfaces`, 1e6 pixels): 5e-4 of the row."""
    ref = np.asarray(ref, np.float64)
    rowmax = np.abs(ref).reshape(len(ref), -1).max(axis=1)
    r = np.maximum(np.asarray(radii, np.float64), 1.0)
    slack = factor * EPS32 * np.sqrt(np.pi) * r * rowmax
    return slack.reshape((len(ref),) + (1,) * (ref.ndim - 1)) * np.ones_like(ref)


def means2d_slack(v_xy, conics, radii, factor=8.0) -> np.ndarray:
    """footprint_slack for the screen-space gradient, with the cancellation of its last step: dL/dx = A Sx + B Sy, dL/dy = B Sx + C Sy
    ((A, B, C) the conic, (Sx, Sy) the first moments of dL/dsigma over the footprint).  Along a needle the two products are each far
    larger than their sum; the moments carry the rounding of a sum over the footprint (eps32 sqrt(pixels)), so the result carries
    factor * eps32 * sqrt(pixels) * (|A Sx| + |B Sy|) — the moments are recovered from the oracle's gradient as cov2D (vx, vy)."""
    v, c = np.asarray(v_xy, np.float64), np.asarray(conics, np.float64)
    A, B, C = c[:, 0], c[:, 1], c[:, 2]
    det = np.where(A * C - B * B > 0, A * C - B * B, 1.0)
    a, b, cc = C / det, -B / det, A / det
    sx, sy = a * v[:, 0] + b * v[:, 1], b * v[:, 0] + cc * v[:, 1]
    terms = np.stack([np.abs(A * sx) + np.abs(B * sy), np.abs(B * sx) + np.abs(C * sy)], axis=1)
    r = np.maximum(np.asarray(radii, np.float64), 1.0)
    return factor * EPS32 * np.sqrt(np.pi) * r[:, None] * terms


def assert_close_scaled(got, ref, rel, name="", frac_ok=1.0, rel_all=None, frac_1e2=None, outliers=0, rel_outliers=0.5, slack=None):
    """ratio = |got - ref| / (|ref| + rms(ref)) elementwise, with three tiers:
         ratio <= rel       for at least `frac_ok` of the elements (the claimed tolerance);
         ratio <= 1e-2      for at least `frac_1e2` of them (default: all when rel_all <= 1e-2, else 1 - 5e-5; measured up to 3e-5);
         ratio <= rel_all   for EVERY element (the hard cap on the excused tail; None: no cap unless frac_ok == 1).
    Why a tail exists at all: a splat whose alpha meets the 1/255 skip threshold (or a pixel its transmittance stop) within the
    ~1e-6 relative difference between the hardware exp/rcp and the fp64 oracle gains or loses ONE pixel's whole contribution; for
    a splat seen by few pixels that is a sizeable share of a small gradient.  The tiers keep such flips rare (counted, printed)
    and bounded, while a systematically wrong gradient (ratio ~ 1 or more on many elements) fails all of them."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if ref.size == 0:
        return
    assert np.isfinite(got).all(), f"{name}: non-finite values"
    rms = float(np.sqrt(np.mean(ref * ref))) + 1e-30
    # `slack` (cov_chain_slack): an absolute, per-element allowance on top of rel * (|ref| + rms) — the error is judged against
    # rel * (|ref| + rms) + slack, expressed here as a larger denominator so that the tiers below apply unchanged
    ratio = np.abs(got - ref) / (np.abs(ref) + rms + (0.0 if slack is None else np.asarray(slack, np.float64) / rel))
    bad = ratio > rel
    worst = float(ratio.max())
    n2 = int((ratio > 1e-2).sum())
    if bad.any():
        print(f"[tail] {name}: {int(bad.sum())} of {bad.size} elements outside rel={rel:g}, {n2} outside 1e-2 (worst {worst:.3e})")
    frac = 1.0 - bad.mean()
    assert frac >= frac_ok, f"{name}: {bad.sum()} / {bad.size} outside rel={rel} (worst {worst:.3e})"
    if rel_all is not None:
        n_over = int((ratio > rel_all).sum())
        if n_over:
            print(f"[tail] {name}: {n_over} element(s) beyond the cap {rel_all:g} (worst {worst:.3e}); allowed: {outliers} up to {rel_outliers:g}")
        # `outliers` elements (a counted handful among millions: single flipped decisions on splats that few pixels see) may pass the
        # cap, up to `rel_outliers`
        assert n_over <= outliers and worst <= (rel_outliers if outliers else rel_all), \
            f"{name}: worst element {worst:.3e}, {n_over} beyond the tail cap {rel_all:g} (allowed {outliers} up to {rel_outliers:g})"
        if rel_all > 1e-2 and rel < 1e-2:
            allowed = (5e-5 if frac_1e2 is None else 1.0 - frac_1e2) * ratio.size
            assert n2 <= max(allowed, 1.0), f"{name}: {n2} elements outside 1e-2 (allowed {allowed:.1f} of {ratio.size})"


def assert_pixels_close(got, ref, tol=1e-5, frac_ok=0.999, tol_all=4e-3, name="render"):
    """|got - ref| <= tol for at least frac_ok of the pixels and <= tol_all for EVERY pixel.  The tail bound is the size of ONE
    flipped discrete decision: a splat whose alpha meets the 1/255 skip threshold within the ~1e-6 relative difference between
    the hardware exp/rcp and fp64 is blended by one side and skipped by the other, which moves the pixel by
    alpha T |c - C_behind| <= 1/255 = 3.9e-3 for colours in [0, 1] (measured maxima at 1-6 M splats: 1.1e-3 ... 2.3e-3).
    Counts are reported."""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    bad = d > tol
    if bad.any():
        print(f"[tail] {name}: {int(bad.sum())} of {bad.size} values outside {tol:g} (max {d.max():.3e})")
    assert 1.0 - bad.mean() >= frac_ok, f"{name}: {bad.sum()} / {bad.size} outside {tol} (max {d.max():.3e})"
    assert d.max() <= tol_all, f"{name}: max |diff| {d.max():.3e} exceeds the tail bound {tol_all:g}"


# ---------------------------------------------------------------------------------------------
# attribution of the free-running tests' tail: not "at most so many elements may be off" but "an element that is
# off belongs to a splat that a decision the fp32 pipeline may legitimately take the other way can reach"
# ---------------------------------------------------------------------------------------------
def fragile_rows(mode, r, W, H, bg, opacities=None, gpu_radii=None, tile=16, input_eps=4 * 2.0 ** -24, order_tol=4 * 2.0 ** -24):
    """(rows [N] bool, fragile_px [H,W] bool) for an oracle render `r` (oracle.render_gsplat / render_inria: its per-splat values and
    ITS lists).  A row is fragile when
      * the splat is — or within the oracle's 2e-5 margin could be — blended in a pixel in which some discrete decision (1/255 skip,
        transmittance stop, alpha clamp) sits within that margin of its threshold, or in which two blended splats are within a few
        fp32 ulps of each other in depth (their order is the sort's decision on fp32 keys) — oracle.fragile_splats / fragile_order:
        one flipped decision there moves the pixel by up to 1/255 and the gradient terms of EVERY splat blended in it; or
      * the two sides disagree on the splat's integer extent (`gpu_radii` != the oracle's radii: ceil(3 sqrt(lambda)) within an ulp
        of an integer, or the visibility test itself) — its tile lists differ.
    Everything else has identical discrete decisions on both sides and must meet the plain tolerance."""
    from oracle import gsplat_oracle as O
    xy = r["xys"] if "xys" in r else r["xy"]
    op = r["opacities"] if "opacities" in r else opacities
    op = op.detach().reshape(-1) if hasattr(op, "detach") else np.asarray(op).reshape(-1)
    _, _, _, frag = O.composite_fwd(mode, xy.detach(), r["conics"].detach(), r["rgbs"].detach(), op, bg, W, H, r["offsets"], r["flatten_ids"], tile=tile,
                                    input_eps=input_eps)
    # ... and the depth ORDER of two blended splats whose depths agree to a few fp32 ulps (the sort key is the fp32 depth)
    frag = O.fragile_order(mode, xy.detach(), r["conics"].detach(), op, r["depths"].detach(), W, H, r["offsets"], r["flatten_ids"], fragile_px=frag, tile=tile,
                           tol_rel=order_tol)
    differ = None
    if gpu_radii is not None:
        ref_radii = np.asarray(r["radii"].detach().cpu().numpy() if hasattr(r["radii"], "detach") else r["radii"]).reshape(-1)
        got_radii = np.asarray(gpu_radii.detach().cpu().numpy() if hasattr(gpu_radii, "detach") else gpu_radii).reshape(-1)
        differ = ref_radii != got_radii
        # a splat whose extent differs sits in other tiles' lists on the two sides: every pixel it can reach there (alpha at 3 sigma is
        # up to 0.011 o: above 1/255 for an opaque splat) composites a different list — flagged, so that the splats blended with it
        # count as reachable too
        xyn = xy.detach().cpu().numpy()
        for g in np.nonzero(differ)[0]:
            rad = int(max(ref_radii[g], got_radii[g])) + 1
            x0, x1 = int(max(np.floor(xyn[g, 0]) - rad, 0)), int(min(np.ceil(xyn[g, 0]) + rad + 1, W))
            y0, y1 = int(max(np.floor(xyn[g, 1]) - rad, 0)), int(min(np.ceil(xyn[g, 1]) + rad + 1, H))
            if x1 > x0 and y1 > y0:
                frag[y0:y1, x0:x1] = 1
    rows = O.fragile_splats(mode, xy.detach(), r["conics"].detach(), op, W, H, r["offsets"], r["flatten_ids"], frag, tile=tile, input_eps=input_eps)
    if differ is not None:
        rows = rows | differ
    return rows, frag != 0


def assert_close_attributed(got, ref, rel, name, rows, frac_ok=0.995, rel_all=0.5, slack=None, quiet=False, rel_firm=5e-3, frac_firm=2.5e-4):
    """The free-running gradient check WITH attribution.  ratio = |got - ref| / (|ref| + rms(ref) [+ slack / rel]) per element;
      1. EVERY element with ratio > `rel_firm` (5e-3: a hundredth of the cap on the fragile rows) lies in a row of `rows`
         (hip_helpers.fragile_rows: a decision the fp32 pipeline may legitimately take the other way reaches that splat) — asserted;
         and of the elements OUTSIDE those rows at most `frac_firm` (2.5e-4; at least one) lie between rel and rel_firm: with identical
         decisions what is left is the SMOOTH effect of the few-ulp differences between the per-splat inputs the two sides composite
         (a free-running oracle projects in fp64).  Measured (gpurun_out r20, profiles/r20_attribution.txt): scenes of 3-20 k splats —
         none, worst unreachable element 9e-5; S-800-100k (3-pixel splats, the most sensitive) 22 of 120 k such elements, worst 5.3e-4;
         1-6 M splats at 1080p 7-60 of 3-288 M, worst 8.5e-4; 5 M at SH degree 0 149 of 14 M, worst 3.0e-3.  The locked tests, which
         composite AT the GPU's values, hold every such element to 1e-4;
      2. the fragile rows themselves stay bounded: at least `frac_ok` of ALL elements within rel, every element within `rel_all`
         (one flipped 1/255 decision on a splat that few pixels see is a sizeable share of a small gradient, not more);
      3. printed, not asserted: how many elements rely on the attribution, and the quantiles of the PURE relative error
         |got - ref| / |ref| over the elements with |ref| > 1e-3 rms (north_star says "1e-4 rel": read it off here)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if ref.size == 0:
        return
    assert np.isfinite(got).all(), f"{name}: non-finite values"
    rows = np.asarray(rows, bool).reshape(-1)
    assert rows.shape[0] == ref.shape[0], (name, rows.shape, ref.shape)
    rms = float(np.sqrt(np.mean(ref * ref))) + 1e-30
    err = np.abs(got - ref)
    ratio = err / (np.abs(ref) + rms + (0.0 if slack is None else np.asarray(slack, np.float64) / rel))
    bad = ratio > rel
    row_of = np.broadcast_to(rows.reshape((-1,) + (1,) * (ref.ndim - 1)), ref.shape)
    unattributed = (ratio > rel_firm) & ~row_of
    band = bad & ~row_of & ~unattributed
    big = np.abs(ref) > 1e-3 * rms
    pure = err[big] / np.abs(ref[big])
    q = np.quantile(pure, [0.5, 0.99, 0.999]) if pure.size else [0, 0, 0]
    if not quiet:
        print(f"[attributed] {name}: {int(bad.sum())} of {bad.size} elements beyond {rel:g}: {int((bad & row_of).sum())} in the {int(rows.sum())} fragile rows of "
              f"{rows.size}, {int(band.sum())} outside them up to {rel_firm:g}, {int(unattributed.sum())} outside them beyond it; worst ratio "
              f"{float(ratio.max()):.2e} (non-fragile rows {float(ratio[~row_of].max()) if (~row_of).any() else 0.0:.2e}); "
              f"pure |d|/|ref| p50 {q[0]:.1e} p99 {q[1]:.1e} p99.9 {q[2]:.1e}")
    if unattributed.any():
        i = int(np.argmax(np.where(unattributed, ratio, 0.0)))
        row = np.unravel_index(i, ref.shape)[0]
        raise AssertionError(f"{name}: {int(unattributed.sum())} element(s) beyond {rel_firm:g} in rows no fragile decision reaches; worst: row {row}, "
                             f"got {got.flat[i]:.6e} ref {ref.flat[i]:.6e} ratio {ratio.flat[i]:.3e} (rms {rms:.3e})")
    n_firm = int((~row_of).sum())
    assert int(band.sum()) <= max(frac_firm * n_firm, 1.0), \
        f"{name}: {int(band.sum())} of {n_firm} elements outside the fragile rows lie between {rel:g} and {rel_firm:g} (allowed {max(frac_firm * n_firm, 1.0):.1f})"
    assert 1.0 - bad.mean() >= frac_ok, f"{name}: {int(bad.sum())} / {bad.size} outside rel={rel} (fragile rows included; worst {float(ratio.max()):.3e})"
    assert float(ratio.max()) <= rel_all, f"{name}: worst element {float(ratio.max()):.3e} beyond the cap {rel_all:g} on a fragile row"


def assert_pixels_attributed(got, ref, fragile_px, tol=1e-5, tol_all=4e-3, name="render"):
    """EVERY pixel the oracle does not flag within `tol`; the flagged ones within one 8-bit step.  got / ref: [3,H,W] or [H,W,3] with
    fragile_px [H,W]."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d = np.abs(got - ref)
    d = d.max(axis=0) if d.shape[0] == 3 and d.ndim == 3 and d.shape[1:] == fragile_px.shape else d.max(axis=-1)
    firm = ~np.asarray(fragile_px, bool)
    worst_firm, worst = float(d[firm].max()) if firm.any() else 0.0, float(d.max())
    print(f"[attributed] {name}: {int((d > tol).sum())} of {d.size} pixels beyond {tol:g}; {int((~firm).sum())} flagged; worst unflagged {worst_firm:.2e}, worst {worst:.2e}")
    assert worst_firm <= tol, f"{name}: an unflagged pixel differs by {worst_firm:.3e} (> {tol:g})"
    assert worst <= tol_all, f"{name}: max |diff| {worst:.3e} exceeds the tail bound {tol_all:g}"


def assert_pipeline_attributed(mode, r, W, H, bg, render, pairs, opacities=None, gpu_radii=None, pixel_tol=1e-5, rel=1e-4, slack=None, **kw):
    """A whole pipeline against a FREE-RUNNING oracle render `r`: every pixel the oracle does not flag within `pixel_tol` (flagged ones
    within one 8-bit step), and every gradient of `pairs` = [(name, got [N,...], ref [N,...]), ...] through `assert_close_attributed`
    with the rows `fragile_rows` derives from r.  `slack`: {name: per-element allowance} (the conditioning of needles).
    pixel_tol None: the pixel tiers of `assert_pixels_close` instead (scenes with needles: sigma of a 600-pixel splat is a difference of
    terms of 1e5, and a few ulps on its conic move alpha by per cent WITHOUT any decision flipping — the locked tests own those)."""
    rows, frag = fragile_rows(mode, r, W, H, bg, opacities=opacities, gpu_radii=gpu_radii)
    print(f"[attributed] {int(frag.sum())} of {frag.size} pixels and {int(rows.sum())} of {rows.size} splats reachable by a fragile decision")
    if render is not None:
        ref_img = r["render"].detach().numpy() if hasattr(r["render"], "detach") else np.asarray(r["render"])
        if pixel_tol is None:
            assert_pixels_close(render, ref_img)
        else:
            assert_pixels_attributed(render, ref_img, frag, tol=pixel_tol)
    for name, got, ref in pairs:
        assert_close_attributed(got, ref, rel, name, rows, slack=None if slack is None else slack.get(name), **kw)
    return rows, frag


def guard_library_blocks(monkeypatch, guard=4096, fill=None):
    """Every block the library asks its allocation call-back for (`ops._frame.allocate`) handed out between two bands of 0xA5, `guard`
    bytes each (the inner block stays 256-byte aligned, as torch's own blocks are), and pre-filled with `fill` when one is given.
    Returns the list of (tag, bytes, outer block) handed out, for `check_guard_bands`."""
    from gspl_amd.ops import _frame
    outers = []

    def allocate(nbytes, device, tag):
        size = ((nbytes + 255) // 256 * 256 + 2 * guard,)
        outer = torch.empty(size, dtype=torch.uint8, device=device) if fill is None else torch.full(size, fill, dtype=torch.uint8, device=device)
        outer[:guard] = 0xA5
        outer[guard + nbytes:] = 0xA5
        outers.append((tag, nbytes, outer))
        return outer[guard:guard + nbytes]

    monkeypatch.setattr(_frame, "allocate", allocate)
    return outers


def check_guard_bands(outers, what, guard=4096):
    """Both bands of every block `guard_library_blocks` handed out are intact; returns how many blocks there were."""
    torch.cuda.synchronize()
    assert outers, f"{what}: nothing was allocated through the call-back"
    for tag, n, outer in outers:
        assert bool((outer[:guard] == 0xA5).all()), f"{what}: a write BELOW block {tag} ({n} bytes)"
        assert bool((outer[guard + n:] == 0xA5).all()), f"{what}: a write ABOVE block {tag} ({n} bytes)"
    return len(outers)

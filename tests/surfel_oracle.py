"""fp64 oracle of the 2D Gaussian Splatting (surfel) rasterizer of csrc/surfel.hip (the published 2DGS rule restated in the Inria
conventions; include/gspl_hip.h section 6c).  Dense: every pixel evaluates, in stable depth order, every splat whose tile rect covers
the pixel's 16x16 tile.  Gradients come from autograd, with the two conventions of the HIP backward written out:
  * the 0.99 alpha clamp is straight-through (value min(0.99, a), derivative 1);
  * `means2D.grad` is upstream's densification proxy: a zero tensor is added to Tu.z / Tv.z where the compositing reads them (not in
    the centre formula), and its gradient, times Tw.z W/2 (H/2), is the proxy.
`render` also returns, per pixel, whether a decision fp32 may take differently lies within a stated margin (`flagged`), and the
splats whose own decision is the fragile one (`flagged_rows`)."""

import numpy as np
import torch

from oracle import gsplat_oracle as O

C_CUT = 3.0
FILTER = 0.707106
FILTER_INV_SQ = 1.0 / (FILTER * FILTER)
NEAR, FAR = 0.2, 100.0
M_SCALE = FAR / (FAR - NEAR)
# margins of the fragile decisions
ALPHA_MIN_TOL = 1e-6        # |o G - 1/255| (fp32 carries ~1e-8 there for a well-conditioned intersection)
T_STOP_TOL = 2e-8           # |T (1 - alpha) - 1e-4| (2e-4 relative: fp32 carries ~1e-5 after a few hundred splats)
T_MED_TOL = 1e-5            # |T - 0.5| at the median switch
RHO_TOL = 1e-4              # |rho3 - rho2| relative to 1 + rho2
Z_TOL = 1e-5                # |z - 0.2|
PZ_COND = 1e-3              # |p.z| < PZ_COND |k| |l|: an edge-on surfel (ill-conditioned intersection)
COS_TOL = 1e-5              # |cos| relative to |p_view|: the normal's flip
RADIUS_TOL = 1e-5           # |h - round(h)| relative to h: the radius's ceil


def _normalize_quat(q):
    return q / q.norm(dim=-1, keepdim=True)


def preprocess(means, scales, quats, viewmatrix, projmatrix, width, height, scale_modifier=1.0, proxy=None):
    """Per splat: dict(Tu, Tv, Tw [N,3] (compositing's copies carry the proxy zeros), centre [N,2], normal [N,3] (view, flipped),
    depth [N], radii [N] i32, mask [N])."""
    dt = means.dtype
    V, P = viewmatrix.to(dt), projmatrix.to(dt)
    N = means.shape[0]
    pv = means @ V[:3, :3] + V[3, :3]
    R = O.quat_to_rotmat(_normalize_quat(quats))
    su, sv = scales[:, 0] * scale_modifier, scales[:, 1] * scale_modifier
    tu, tv, nw = R[:, :, 0] * su[:, None], R[:, :, 1] * sv[:, None], R[:, :, 2]
    Nm = torch.tensor([[width / 2, 0, 0], [0, height / 2, 0], [0, 0, 0], [(width - 1) / 2, (height - 1) / 2, 1]], dtype=dt)
    Q = P @ Nm                                                     # [4,3]
    a, b = Q[:3], Q[3]
    Tx = torch.stack([tu @ a, tv @ a, means @ a + b], dim=1)      # [N,3 (u v w rows), 3 (x y w)]
    Tu, Tv, Tw = Tx[:, :, 0], Tx[:, :, 1], Tx[:, :, 2]
    t = torch.tensor([C_CUT ** 2, C_CUT ** 2, -1.0], dtype=dt)
    d = (t * Tw * Tw).sum(-1)
    ok = (pv[:, 2].detach() > NEAR) & (d.detach() != 0)
    d_safe = torch.where(ok, d, torch.ones_like(d))
    f = t / d_safe[:, None]
    cx, cy = (f * Tu * Tw).sum(-1), (f * Tv * Tw).sum(-1)
    with torch.no_grad():
        hx = torch.sqrt(torch.clamp_min(cx ** 2 - (f * Tu * Tu).sum(-1), 1e-4))
        hy = torch.sqrt(torch.clamp_min(cy ** 2 - (f * Tv * Tv).sum(-1), 1e-4))
        hmax = torch.maximum(torch.maximum(hx, hy), torch.full_like(hx, C_CUT * FILTER))
        radius = torch.ceil(hmax)
        # the ceil is a decision fp32 may take differently when the extent lies within RADIUS_TOL of an integer
        radius_fragile = (hmax - torch.round(hmax)).abs() < RADIUS_TOL * hmax
    nv = nw @ V[:3, :3]
    cos = -(pv * nv).sum(-1).detach()
    # the flip towards the camera is a decision fp32 may take differently for a nearly edge-on surfel
    cos_fragile = cos.abs() < COS_TOL * pv.detach().norm(dim=-1)
    ok = ok & (cos != 0)
    sign = torch.where(cos < 0, -1.0, 1.0).to(dt)
    nv = nv * sign[:, None]
    centre = torch.stack([cx, cy], dim=-1)
    radii = torch.where(ok, radius, torch.zeros_like(radius)).to(torch.int32)
    # the Inria tile rect; an empty rect culls
    minx, miny, maxx, maxy = O.tile_rects(O.MODE_INRIA, centre.detach().numpy(), radii.numpy(), width, height)
    empty = torch.from_numpy((maxx - minx) * (maxy - miny) <= 0)
    radii = torch.where(empty, torch.zeros_like(radii), radii)
    mask = radii > 0
    if proxy is not None:
        zu, zv = proxy
        zero = torch.zeros_like(zu)
        Tu = Tu + torch.stack([zero, zero, zu], dim=-1)
        Tv = Tv + torch.stack([zero, zero, zv], dim=-1)
    return dict(Tu=Tu, Tv=Tv, Tw=Tw, centre=centre, normal=nv, depth=pv[:, 2], radii=radii, mask=mask, radius_fragile=radius_fragile & ok, cos_fragile=cos_fragile)


def _composite_tile(pre, ids, colors, opac, xs, ys):
    """Pixels (xs, ys) [P] against splats `ids` [K] in order.  Returns per-pixel tensors."""
    dt = colors.dtype
    if ids.numel() == 0:
        P = xs.numel()
        z1, z3 = torch.zeros(P, dtype=dt), torch.zeros((P, 3), dtype=dt)
        zi, zb = torch.zeros(P, dtype=torch.int64), torch.zeros(P, dtype=torch.bool)
        return dict(color=z3, T=torch.ones(P, dtype=dt), depth=z1, normal=z3, median=z1, dist=z1, flagged=zb, rows=ids,
                    pairs_3d=0, pairs_lowpass=0, pairs_clamped=0, contributors=zi, last=zi, stopped=zb, first_clamped=zb, list_length=0)
    Tu, Tv, Tw = pre["Tu"][ids], pre["Tv"][ids], pre["Tw"][ids]
    cen, nrm, col, o = pre["centre"][ids], pre["normal"][ids], colors[ids], opac[ids]
    x, y = xs[:, None, None].to(dt), ys[:, None, None].to(dt)
    k = x * Tw[None] - Tu[None]
    l = y * Tw[None] - Tv[None]
    p = torch.cross(k, l, dim=-1)                                  # [P,K,3]
    pz = p[..., 2]
    v1 = pz.detach() != 0
    pz_s = torch.where(v1, pz, torch.ones_like(pz))
    s = p[..., :2] / pz_s[..., None]
    rho3 = (s * s).sum(-1)
    dlt = cen[None] - torch.stack([xs, ys], dim=-1).to(dt)[:, None, :]
    rho2 = FILTER_INV_SQ * (dlt * dlt).sum(-1)
    use3 = rho3.detach() <= rho2.detach()
    z = torch.where(use3, s[..., 0] * Tw[None, :, 0] + s[..., 1] * Tw[None, :, 1] + Tw[None, :, 2], Tw[None, :, 2].expand_as(rho3))
    v2 = z.detach() >= NEAR
    rho = torch.where(use3, rho3, rho2)
    a_raw = o[None] * torch.exp(-0.5 * rho)
    alpha = a_raw - torch.clamp_min(a_raw - 0.99, 0.0).detach()       # straight-through clamp
    keep = v1 & v2 & (alpha.detach() >= 1.0 / 255.0)
    ak = torch.where(keep, alpha, torch.zeros_like(alpha))
    Tincl = torch.cumprod(1 - ak.detach(), dim=1)
    stop = keep & (Tincl < 1e-4)
    comp = keep & (torch.cumsum(stop.to(torch.int64), dim=1) == 0)
    ac = torch.where(comp, alpha, torch.zeros_like(alpha))
    one = torch.ones_like(ac[:, :1])
    Tb = torch.cumprod(torch.cat([one, 1 - ac[:, :-1]], dim=1), dim=1)     # T in front of each splat
    w = ac * Tb
    Tf = Tb[:, -1] * (1 - ac[:, -1])
    zc = torch.where(comp, z, torch.ones_like(z))
    m = M_SCALE * (1 - NEAR / zc)
    wm, wm2 = w * m, w * m * m
    M1b = torch.cumsum(wm, dim=1) - wm
    M2b = torch.cumsum(wm2, dim=1) - wm2
    dist = (w * (m * m * (1 - Tb) + M2b - 2 * m * M1b)).sum(1)
    medsel = comp & (Tb.detach() > 0.5)
    # the median contributor: the last composited splat with T > 0.5 in front of it
    idx = torch.arange(ac.shape[1])[None].expand_as(ac)
    last_med = torch.where(medsel, idx, torch.full_like(idx, -1)).max(dim=1).values
    has_med = last_med >= 0
    med = torch.where(has_med, z.gather(1, last_med.clamp_min(0)[:, None])[:, 0], torch.zeros_like(Tf))
    out = dict(color=(w[..., None] * col[None]).sum(1), T=Tf, depth=(w * z).sum(1), normal=(w[..., None] * nrm[None]).sum(1),
               median=med, dist=dist)
    # fragile decisions, up to and including the stop: per (pixel, splat), the splat whose own decision fp32 may take differently
    with torch.no_grad():
        upto = torch.cumsum(stop.to(torch.int64), dim=1) - stop.to(torch.int64) == 0
        cand = v1 & v2 & upto
        fk = cand & ((a_raw - 1.0 / 255.0).abs() < ALPHA_MIN_TOL)
        fk |= keep & upto & ((Tb * (1 - alpha) - 1e-4).abs() < T_STOP_TOL)
        fk |= comp & ((Tb - 0.5).abs() < T_MED_TOL)
        vis = v1 & upto & (a_raw >= 0.5 / 255.0)
        fk |= vis & ((rho3 - rho2).abs() < RHO_TOL * (1 + rho2))
        fk |= v1 & upto & (a_raw >= 0.5 / 255.0) & ((z - NEAR).abs() < Z_TOL)
        cond = pz.abs() < PZ_COND * k.norm(dim=-1) * l.norm(dim=-1)
        fk |= cond & upto & (o[None] * torch.exp(-0.5 * rho2) >= 0.5 / 255.0)
        fk |= vis & pre["cos_fragile"][ids][None]
        fl = fk.any(1)
        touched = fk.any(0)
        # statistics of the composited (pixel, splat) pairs: which paths a scene reaches
        pos = idx + 1
        out["pairs_3d"] = int((comp & use3).sum())
        out["pairs_lowpass"] = int((comp & ~use3).sum())
        out["pairs_clamped"] = int((comp & (a_raw > 0.99)).sum())
        out["contributors"] = comp.sum(1)
        out["last"] = torch.where(comp, pos, torch.zeros_like(pos)).max(dim=1).values      # one past the last contributor's list position
        out["stopped"] = stop.any(1)
        first = torch.where(comp, idx, torch.full_like(idx, ac.shape[1])).min(dim=1).values
        out["first_clamped"] = comp.any(1) & (a_raw.gather(1, first.clamp_max(ac.shape[1] - 1)[:, None])[:, 0] > 0.99)
        out["list_length"] = int(ids.numel())
    out["flagged"] = fl
    out["rows"] = ids[touched]
    return out


def render(means, scales, quats, opacities, sh_coeffs, degree, viewmatrix, projmatrix, campos, width, height, background,
           scale_modifier=1.0, colors_precomp=None, proxy=None, pixels=None):
    """dict(render [3,H,W], allmap [7,H,W], radii [N], flagged [H,W] bool, means2d_scale [N,2] (Tw.z W/2, Tw.z H/2: the proxy's
    factors), pre (the preprocess dict)).  `proxy`: (zu, zv) zero tensors [N] whose gradients give the densification proxy.
    Statistics of the composited (pixel, splat) pairs, for tests that must know which paths a scene reaches: pairs_3d / pairs_lowpass /
    pairs_clamped (counts: the ray-splat intersection, the screen-space low-pass, a raw alpha above 0.99), contributors [H,W] (per
    pixel), last [H,W] (the position in the tile's list one past the last contributor; 0: none), stopped [H,W] (the pixel met the
    transmittance stop), first_clamped [H,W] (the first contributor's raw alpha is above 0.99), list_lengths [tiles_y, tiles_x]."""
    dt = means.dtype
    pre = preprocess(means, scales, quats, viewmatrix, projmatrix, width, height, scale_modifier, proxy)
    mask = pre["mask"]
    if colors_precomp is None:
        rgb = O.sh_colors(degree, sh_coeffs, means, campos, detach_dirs=False)
    else:
        rgb = colors_precomp.to(dt)
    rgb = torch.where(mask[:, None], rgb, torch.zeros((), dtype=dt))
    opac = opacities.reshape(-1)
    tw, th = (width + 15) // 16, (height + 15) // 16
    minx, miny, maxx, maxy = O.tile_rects(O.MODE_INRIA, pre["centre"].detach().numpy(), pre["radii"].numpy(), width, height)
    order = np.argsort(pre["depth"].detach().numpy().astype(np.float32), kind="stable")
    chans = {k: torch.zeros((c, height, width), dtype=dt) for k, c in (("color", 3), ("depth", 1), ("normal", 3), ("median", 1), ("dist", 1))}
    Tmap = torch.ones((height, width), dtype=dt)
    flagged = torch.zeros((height, width), dtype=torch.bool)
    parts = []
    if pixels is None:
        tiles = [(ty, tx) for ty in range(th) for tx in range(tw)]
    else:
        pys, pxs = torch.nonzero(pixels, as_tuple=True)
        tiles = sorted(set(zip((pys // 16).tolist(), (pxs // 16).tolist())))
    for ty, tx in tiles:
        if True:
            x0, y0 = tx * 16, ty * 16
            xs_t = torch.arange(x0, min(x0 + 16, width))
            ys_t = torch.arange(y0, min(y0 + 16, height))
            yy, xx = torch.meshgrid(ys_t, xs_t, indexing="ij")
            xs, ys = xx.reshape(-1), yy.reshape(-1)
            if pixels is not None:
                sel = pixels[ys, xs]
                xs, ys = xs[sel], ys[sel]
                if xs.numel() == 0:
                    continue
            covers = (minx[order] <= tx) & (tx < maxx[order]) & (miny[order] <= ty) & (ty < maxy[order])
            ids = torch.from_numpy(order[covers].astype(np.int64))
            r = _composite_tile(pre, ids, rgb, opac, xs, ys)
            parts.append((xs, ys, r))
    # assemble without in-place writes into leaves that need gradients
    flagged_rows = torch.zeros(means.shape[0], dtype=torch.bool)
    stats = {k: 0 for k in ("pairs_3d", "pairs_lowpass", "pairs_clamped")}
    per_pixel = {k: torch.zeros((height, width), dtype=t) for k, t in (("contributors", torch.int64), ("last", torch.int64), ("stopped", torch.bool),
                                                                      ("first_clamped", torch.bool))}
    list_lengths = torch.zeros((th, tw), dtype=torch.int64)
    for xs, ys, r in parts:
        flagged[ys, xs] = r["flagged"]
        flagged_rows[r["rows"]] = True
        for k in stats:
            stats[k] += r[k]
        for k, img in per_pixel.items():
            img[ys, xs] = r[k]
        list_lengths[int(ys[0]) // 16, int(xs[0]) // 16] = r["list_length"]
    def assemble(fn, c):
        img = torch.zeros((c, height * width), dtype=dt)
        for xs, ys, r in parts:
            img = img.index_put((torch.arange(c)[:, None], (ys * width + xs)[None]), fn(r), accumulate=False)
        return img.reshape(c, height, width)
    T = assemble(lambda r: r["T"][None], 1)
    if pixels is None:
        T = T
    else:
        T = torch.where(pixels[None], T, torch.ones_like(T))
    bgc = background.reshape(-1).to(dt)
    color = assemble(lambda r: r["color"].T, 3) + T * bgc[:, None, None]
    allmap = torch.cat([assemble(lambda r: r["depth"][None], 1), 1 - T, assemble(lambda r: r["normal"].T, 3),
                        assemble(lambda r: r["median"][None], 1), assemble(lambda r: r["dist"][None], 1)], dim=0)
    scale2 = torch.stack([pre["Tw"][:, 2] * width / 2, pre["Tw"][:, 2] * height / 2], dim=-1).detach()
    return dict(render=color, allmap=allmap, radii=pre["radii"], flagged=flagged, flagged_rows=flagged_rows, means2d_scale=scale2, pre=pre, rgb=rgb,
                list_lengths=list_lengths, **stats, **per_pixel)


def render_with_grads(means, scales, quats, opacities, sh_coeffs, degree, viewmatrix, projmatrix, campos, width, height, background,
                      v_color, v_allmap, scale_modifier=1.0, colors_precomp=None):
    """Forward + autograd backward for given output gradients.  Returns (result dict, grads dict) with the means2D proxy."""
    leaves = {"means": means, "scales": scales, "quats": quats, "opacities": opacities}
    if colors_precomp is None:
        leaves["shs"] = sh_coeffs
    else:
        leaves["colors_precomp"] = colors_precomp
    leaves = {k: v.detach().double().requires_grad_(True) for k, v in leaves.items()}
    N = means.shape[0]
    zu = torch.zeros(N, dtype=torch.float64, requires_grad=True)
    zv = torch.zeros(N, dtype=torch.float64, requires_grad=True)
    r = render(leaves["means"], leaves["scales"], leaves["quats"], leaves["opacities"], leaves.get("shs"), degree, viewmatrix.double(),
               projmatrix.double(), campos.double(), width, height, background.double(), scale_modifier=scale_modifier,
               colors_precomp=leaves.get("colors_precomp"), proxy=(zu, zv))
    loss = (r["render"] * v_color.double()).sum() + (r["allmap"] * v_allmap.double()).sum()
    ins = list(leaves.values()) + [zu, zv]
    gs = torch.autograd.grad(loss, ins, allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(v)) for (k, v), g in zip(leaves.items(), gs[:-2])}
    gzu = gs[-2] if gs[-2] is not None else torch.zeros(N, dtype=torch.float64)
    gzv = gs[-1] if gs[-1] is not None else torch.zeros(N, dtype=torch.float64)
    m2 = torch.zeros((N, 3), dtype=torch.float64)
    m2[:, 0] = gzu * r["means2d_scale"][:, 0]
    m2[:, 1] = gzv * r["means2d_scale"][:, 1]
    grads["means2d"] = m2
    return r, grads

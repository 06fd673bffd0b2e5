"""The HIP surfel (2DGS) rasterizer against the fp64 oracle of tests/surfel_oracle.py: forward, every input's gradient, the
deterministic mode, guard bands around every block the allocation call-back hands out, degenerate frames, the plugin's contract and a
short training run with the 2DGS normal and distortion losses."""
import math

import numpy as np
import pytest
import torch

from oracle import gsplat_oracle as O
import surfel_oracle as SO

pytestmark = pytest.mark.gpu

W, H = 96, 72
# colour, alpha and normal on unflagged pixels.  Sub-pixel surfels (extent ~0.05 px) lose ~1e-5 of their alpha in fp32: the per-pixel
# k = x Tw - Tu cancels near the splat's centre (the published rasterizer's formula).  Typical pixels agree to ~1e-6.
TOL = 2e-5


def _special_scene(seed=21, n=600):
    """Random surfels plus edge-on, back-facing, near-plane and screen-filling ones."""
    g = torch.Generator().manual_seed(seed)
    means, scales3, quats, opac, shs = O.synthetic_scene(n, seed=seed)
    scales = scales3[:, :2] * 8
    extra_m, extra_s, extra_q = [], [], []
    half_x = torch.tensor([math.cos(math.pi / 4), math.sin(math.pi / 4), 0.0, 0.0])      # 90 deg about x: plane contains the view axis
    for i in range(6):
        if i < 2:
            extra_m.append([0.6 * (i - 1), 0.2, 0.0]); extra_s.append([0.2, 0.2]); extra_q.append(half_x.tolist())       # edge-on
        extra_m.append([0.25 * (i - 3), -0.3, 0.5]); extra_s.append([0.15, 0.1]); extra_q.append([1.0, 0.0, 0.0, 0.0])  # back-facing
        extra_m.append([0.02 * (i - 3), 0.01 * i, -3.75 + 0.01 * i]); extra_s.append([0.05, 0.05]); extra_q.append([0.0, 1.0, 0.0, 0.0])  # near plane
    extra_m.append([0.0, 0.0, 1.5]); extra_s.append([3.0, 2.5]); extra_q.append([0.9, 0.1, 0.05, 0.0])                    # screen-filling
    k = len(extra_m)
    means = torch.cat([means, torch.tensor(extra_m)])
    scales = torch.cat([scales, torch.tensor(extra_s)])
    quats = torch.cat([quats, torch.tensor(extra_q)])
    opac = torch.cat([opac, torch.rand(k, 1, generator=g) * 0.5 + 0.4])
    shs = torch.cat([shs, torch.randn(k, shs.shape[1], 3, generator=g) * 0.2])
    cam = O.synthetic_camera(W, H, 80.0, 78.0)
    return (means, scales, quats * 1.3, opac, shs), cam


def _settings(cam, bg, mod, dev, degree=3):
    from gspl_amd import ops
    return ops.SurfelRasterizationSettings(image_height=cam["height"], image_width=cam["width"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
                                           bg=bg.to(dev), scale_modifier=mod, viewmatrix=cam["world_to_camera"].to(dev),
                                           projmatrix=cam["full_projection"].to(dev), sh_degree=degree, campos=cam["camera_center"].to(dev))


def _run_hip(params, cam, bg, mod, colour, v_color, v_allmap, cp=None):
    from gspl_amd import ops
    dev = torch.device("cuda:0")
    means, scales, quats, opac, shs = params
    leaves = [t.to(dev).float().requires_grad_(True) for t in (means, scales, quats, opac, cp if colour == "colors_precomp" else shs)]
    m, s, q, o, c = leaves
    screen = torch.zeros_like(m, requires_grad=True)
    kw = dict(colors_precomp=c) if colour == "colors_precomp" else dict(shs=c)
    color, radii, allmap = ops.SurfelGaussianRasterizer(_settings(cam, bg, mod, dev))(means3D=m, means2D=screen, opacities=o, scales=s,
                                                                                      rotations=q, **kw)
    ((color * v_color.to(dev)).sum() + (allmap * v_allmap.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    grads = dict(means=m.grad, scales=s.grad, quats=q.grad, opacities=o.grad, means2d=screen.grad)
    grads["colors_precomp" if colour == "colors_precomp" else "shs"] = c.grad
    return color, radii, allmap, grads


def _oracle(params, cam, bg, mod, colour, v_color, v_allmap, cp=None):
    means, scales, quats, opac, shs = [t.double() for t in params]
    return SO.render_with_grads(means, scales, quats, opac, None if colour == "colors_precomp" else shs, 3, cam["world_to_camera"],
                                cam["full_projection"], cam["camera_center"], cam["width"], cam["height"], bg, v_color, v_allmap,
                                scale_modifier=mod, colors_precomp=cp.double() if colour == "colors_precomp" else None)


def _grad_check(name, got, ref, excused):
    g, rf = got.detach().cpu().double().reshape(ref.shape[0], -1).numpy(), ref.detach().reshape(ref.shape[0], -1).numpy()
    rms = np.sqrt(np.mean(rf * rf)) + 1e-30
    rel = np.abs(g - rf) / (np.abs(rf) + rms)
    bad_rows = (rel > 2e-3).any(1) & ~excused
    assert int(bad_rows.sum()) <= max(1, int(0.002 * rf.shape[0])), f"gradient {name}: {int(bad_rows.sum())} rows off, worst {rel[~excused].max():.3e}"
    assert float(np.median(rel)) <= 1e-4, f"gradient {name}: median {float(np.median(rel)):.3e}"


@pytest.mark.parametrize("colour", ["shs", "colors_precomp"])
def test_surfel_against_fp64_oracle(colour):
    params, cam = _special_scene(seed=21 + (colour == "shs"))
    bg = torch.tensor([0.3, 0.1, 0.6])
    mod = 0.9
    cp = torch.rand(params[0].shape[0], 3, generator=torch.Generator().manual_seed(5))
    gen = torch.Generator().manual_seed(9)
    v_color = torch.randn(3, H, W, generator=gen) * 0.1
    v_allmap = torch.randn(7, H, W, generator=gen) * torch.tensor([0.02, 0.1, 0.1, 0.1, 0.1, 0.02, 5.0])[:, None, None]
    color, radii, allmap, grads = _run_hip(params, cam, bg, mod, colour, v_color, v_allmap, cp)
    r, ref = _oracle(params, cam, bg.double(), mod, colour, v_color.double(), v_allmap.double(), cp)
    fr = r["pre"]["radius_fragile"]
    assert int(fr.sum()) <= 2
    assert torch.equal(radii.cpu()[~fr], r["radii"][~fr]), "radii"
    assert int((radii > 0).sum()) > 300
    flagged = r["flagged"]
    assert int(flagged.sum()) <= 0.01 * H * W, f"{int(flagged.sum())} flagged pixels"
    ok = ~flagged
    c, a = color.cpu().double(), allmap.cpu().double()
    rc, ra = r["render"].detach(), r["allmap"].detach()
    assert float((c - rc).abs()[:, ok].max()) <= TOL
    for ch in (1, 2, 3, 4):      # alpha, normal
        assert float((a[ch] - ra[ch]).abs()[ok].max()) <= TOL, ch
    for ch in (0, 5, 6):         # depth, median: their largest value; distortion: its terms' bound (w m^2 summed, m <= 1), the alpha
        scale = float(ra[1 if ch == 6 else ch].abs().max()) + 1e-12
        assert float((a[ch] - ra[ch]).abs()[ok].max()) <= 1e-5 * scale, ch
    assert float(ra[6].abs().max()) > 0 and float(ra[1].max()) > 0.9
    excused = r["flagged_rows"].numpy()         # splats whose own decision is fragile at some pixel
    assert excused.sum() <= 0.05 * int((radii > 0).sum()), f"{excused.sum()} rows excused"
    for k in ref:
        _grad_check(k, grads[k], ref[k], excused)


def test_surfel_deterministic_mode_is_bit_reproducible():
    from gspl_amd import _lib as L
    params, cam = _special_scene(seed=4)
    bg = torch.tensor([0.2, 0.2, 0.2])
    gen = torch.Generator().manual_seed(2)
    v_color, v_allmap = torch.randn(3, H, W, generator=gen), torch.randn(7, H, W, generator=gen)
    old = L.lib().gspl_set_deterministic(1)
    try:
        runs = [_run_hip(params, cam, bg, 1.0, "shs", v_color, v_allmap)[3] for _ in range(2)]
    finally:
        L.lib().gspl_set_deterministic(old)
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    plain = _run_hip(params, cam, bg, 1.0, "shs", v_color, v_allmap)[3]
    for k in plain:
        assert torch.allclose(plain[k], runs[0][k], rtol=1e-3, atol=1e-6 * float(plain[k].abs().max()) + 1e-12), k


GUARD = 4096


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_surfel_guard_bands(monkeypatch, fill):
    from gspl_amd import _lib as L
    from hip_helpers import check_guard_bands, guard_library_blocks
    outers = guard_library_blocks(monkeypatch, GUARD, fill)
    params, cam = _special_scene(seed=8)
    gen = torch.Generator().manual_seed(1)
    v_color, v_allmap = torch.randn(3, H, W, generator=gen), torch.randn(7, H, W, generator=gen)
    results = []
    for det in (0, 1):
        old = L.lib().gspl_set_deterministic(det)
        try:
            color, radii, allmap, grads = _run_hip(params, cam, torch.tensor([0.1, 0.2, 0.3]), 1.0, "shs", v_color, v_allmap)
        finally:
            L.lib().gspl_set_deterministic(old)
        results.append((color, allmap, grads))
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    tags = {t for t, _, _ in outers}
    assert {L.GSPL_BUF_GEOMETRY, L.GSPL_BUF_IMAGE, L.GSPL_BUF_BINNING, L.GSPL_BUF_LISTS_WORK, L.GSPL_BUF_LISTS, L.GSPL_BUF_SURFEL_ENTRIES} <= tags
    check_guard_bands(outers, "surfel", GUARD)
    # the pre-fill of the blocks does not leak into the results
    ref = _run_hip(params, cam, torch.tensor([0.1, 0.2, 0.3]), 1.0, "shs", v_color, v_allmap)
    assert torch.equal(ref[0], results[0][0]) and torch.equal(ref[2], results[0][1])


@pytest.mark.parametrize("case", ["empty", "all_culled", "one_pixel"])
def test_surfel_degenerate_frames(case):
    from gspl_amd import ops
    dev = torch.device("cuda:0")
    bg = torch.tensor([0.25, 0.5, 0.75], device=dev)
    if case == "one_pixel":
        cam = O.synthetic_camera(1, 1, 1.0)
    else:
        cam = O.synthetic_camera(40, 24, 40.0)
    n = 0 if case == "empty" else 50
    means = torch.rand(n, 3, device=dev) * 0.2
    if case == "all_culled":
        means[:, 2] = -10.0                                     # behind the camera
    leaves = [means.requires_grad_(True), torch.full((n, 2), 0.1, device=dev).requires_grad_(True),
              torch.tensor([[1.0, 0.0, 0.0, 0.0]] * n, device=dev).reshape(n, 4).requires_grad_(True),
              torch.full((n, 1), 0.5, device=dev).requires_grad_(True), torch.rand(n, 3, device=dev).requires_grad_(True)]
    m, s, q, o, c = leaves
    screen = torch.zeros_like(m, requires_grad=True)
    color, radii, allmap = ops.SurfelGaussianRasterizer(_settings(cam, bg, 1.0, dev))(means3D=m, means2D=screen, opacities=o, scales=s,
                                                                                      rotations=q, colors_precomp=c)
    (color.sum() + allmap.sum()).backward()
    torch.cuda.synchronize()
    assert color.shape == (3, cam["height"], cam["width"]) and allmap.shape == (7, cam["height"], cam["width"])
    if case != "one_pixel":
        assert torch.equal(color, bg[:, None, None].expand_as(color)) and bool((allmap == 0).all()) and int((radii > 0).sum()) == 0
    assert all(bool(torch.isfinite(t.grad).all()) for t in leaves)
    if case == "all_culled":
        assert all(float(t.grad.abs().max()) == 0.0 for t in leaves)
    if case == "one_pixel":
        ref = SO.render(*[t.detach().cpu().double() for t in (m, s, q, o)], None, 0, cam["world_to_camera"].double(),
                        cam["full_projection"].double(), cam["camera_center"].double(), 1, 1, bg.cpu().double(), colors_precomp=c.detach().cpu().double())
        assert float((color.cpu().double() - ref["render"]).abs().max()) <= 1e-5


def test_surfel_plugin_contract():
    from fakes import FakeCamera, FakeGaussianModel
    from gspl_amd.renderers import HipVanilla2DGSRenderer
    dev = torch.device("cuda:0")
    params, cam = _special_scene(seed=6)
    means, scales, quats, opac, shs = params
    scales3 = torch.cat([scales, torch.full((scales.shape[0], 1), 1e-3)], dim=1)
    model = FakeGaussianModel(*[t.to(dev) for t in (means, scales3, quats, opac, shs)])
    r = HipVanilla2DGSRenderer(depth_ratio=0.0)
    out = r(FakeCamera(cam, dev), model, torch.tensor([0.0, 0.0, 0.0], device=dev))
    keys = {"render", "viewspace_points", "visibility_filter", "radii", "rend_alpha", "rend_normal", "view_normal", "rend_dist", "surf_depth", "surf_normal"}
    assert set(out) == keys
    for k in keys - {"viewspace_points"}:
        assert out[k].device == dev, k
    assert out["render"].shape == (3, H, W) and out["rend_alpha"].shape == (1, H, W) and out["surf_normal"].shape == (3, H, W)
    loss = out["render"].mean() + out["rend_dist"].mean() + (1 - (out["rend_normal"] * out["surf_normal"]).sum(0)).mean()
    out["viewspace_points"].retain_grad()      # (a non-leaf, as in the reference: `zeros_like(..., requires_grad=True) + 0`)
    loss.backward()
    assert out["viewspace_points"].grad is not None and bool(torch.isfinite(model.means.grad).all())
    assert float(out["viewspace_points"].grad[:, :2].abs().sum()) > 0
    cp = torch.rand(means.shape[0], 3, device=dev)
    out2 = r(FakeCamera(cam, dev), model, torch.tensor([0.0, 0.0, 0.0], device=dev), colors_precomp=cp)
    assert out2["render"].shape == (3, H, W)


def test_surfel_training_with_normal_and_distortion_losses():
    from gspl_amd import ops
    dev = torch.device("cuda:0")
    params, cam = _special_scene(seed=12, n=800)
    target_params, _ = _special_scene(seed=13, n=800)
    bg = torch.tensor([0.0, 0.0, 0.0], device=dev)
    st = _settings(cam, bg, 1.0, dev)
    with torch.no_grad():
        m, s, q, o, c = [t.to(dev).float() for t in target_params]
        target = ops.SurfelGaussianRasterizer(st)(means3D=m, means2D=torch.zeros_like(m), opacities=o, shs=c, scales=s, rotations=q)[0]
    leaves = [t.to(dev).float().clone().requires_grad_(True) for t in params]
    opt = torch.optim.Adam([{"params": [leaves[0]], "lr": 1e-3}, {"params": leaves[1:3], "lr": 5e-3}, {"params": leaves[3:], "lr": 1e-2}])
    from gspl_amd.renderers import HipVanilla2DGSRenderer
    from fakes import FakeCamera
    fcam = FakeCamera(cam, dev)
    losses = []
    for step in range(200):
        m, s, q, o, c = leaves
        screen = torch.zeros_like(m, requires_grad=True)
        color, radii, allmap = ops.SurfelGaussianRasterizer(st)(means3D=m, means2D=screen, opacities=o.clamp(0, 1), shs=c, scales=s.abs(), rotations=q)
        alpha = allmap[1:2]
        depth = torch.nan_to_num(allmap[0:1] / alpha, 0, 0)
        surf_normal = HipVanilla2DGSRenderer.depth_to_normal(fcam, depth).permute(2, 0, 1) * alpha.detach()
        rend_normal = (allmap[2:5].permute(1, 2, 0) @ fcam.world_to_camera[:3, :3].T).permute(2, 0, 1)
        normal_loss = (1 - (rend_normal * surf_normal).sum(0)).mean()
        dist_loss = allmap[6].mean()
        loss = (color - target).abs().mean() + 0.05 * normal_loss + 100.0 * dist_loss
        opt.zero_grad()
        loss.backward()
        for t in leaves:
            assert bool(torch.isfinite(t.grad).all()), step
        opt.step()
        losses.append(float(loss))
    assert all(math.isfinite(v) for v in losses)
    assert np.mean(losses[-20:]) < 0.8 * np.mean(losses[:5]), (losses[:5], losses[-20:])

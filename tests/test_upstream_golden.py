"""Consumes tests/golden/upstream_{inria,gsplat}.npz — outputs and gradients of the upstream CUDA packages the reference
pins (written by tests/golden/make_upstream_golden.py on a machine that has them).  Absent files: skipped, and the
compositing / Inria-preprocess parity stays "unpinned" (DESIGN.md §2).  Present: the oracle (any machine) and the HIP path
(-m gpu) must match them within BASELINE.json's tolerances."""
import os

import numpy as np
import pytest
import torch

from oracle import gsplat_oracle as O
from hip_helpers import assert_close_scaled, assert_pixels_close

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    path = os.path.join(GOLD, name)
    if not os.path.exists(path):
        pytest.skip(f"{name} not generated yet: only an NVIDIA GPU with the upstream CUDA package can write it "
                    "(tests/golden/make_upstream_golden.py)")
    return np.load(path)


def _inputs(cfg):
    n, seed, W, H, fx, fy, mul = cfg
    means, scales, quats, opac, shs = O.synthetic_scene(int(n), seed=int(seed))
    cam = O.synthetic_camera(int(W), int(H), float(fx), float(fy))
    wimg = torch.randn(3, int(H), int(W), generator=torch.Generator().manual_seed(int(seed)))
    return (means, scales * float(mul), quats, opac, shs), cam, wimg, torch.tensor([0.25, 0.5, 0.125])


def _cases(z):
    i = 0
    while f"case{i}_cfg" in z:
        yield i, {k[len(f"case{i}_"):]: z[k] for k in z.files if k.startswith(f"case{i}_")}
        i += 1


def _check(render, grads, gold, names):
    assert_pixels_close(render, gold["render"], tol=1e-5, frac_ok=0.999, tol_all=1e-3)
    for g, n in zip(grads, names):
        assert_close_scaled(g, gold[n], 1e-4, n, frac_ok=0.995, rel_all=0.5)


def test_oracle_matches_upstream_inria():
    for i, gold in _cases(_load("upstream_inria.npz")):
        params, cam, wimg, bg = _inputs(gold["cfg"])
        dl = [t.double().requires_grad_(True) for t in params]
        r = O.render_inria(*dl, 3, cam["world_to_camera"].double(), cam["full_projection"].double(), cam["camera_center"].double(),
                           cam["tanfovx"], cam["tanfovy"], cam["width"], cam["height"], bg.double())
        (r["render"] * wimg.double()).sum().backward()
        _check(r["render"].detach().numpy(), [t.grad.numpy() for t in dl], gold, ("g_means", "g_scales", "g_quats", "g_opac", "g_shs"))
        assert np.mean(r["radii"].numpy() == gold["radii"]) > 0.999


def test_oracle_matches_upstream_gsplat():
    for i, gold in _cases(_load("upstream_gsplat.npz")):
        params, cam, wimg, bg = _inputs(gold["cfg"])
        dl = [t.double().requires_grad_(True) for t in params]
        r = O.render_gsplat(*dl, 3, cam["world_to_camera"].double(), cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["width"], cam["height"],
                            bg.double(), cam["camera_center"].double())
        (r["render"] * wimg.double()).sum().backward()
        _check(r["render"].detach().numpy(), [t.grad.numpy() for t in dl], gold, ("g_means", "g_scales", "g_quats", "g_opac", "g_shs"))
        assert_close_scaled(r["xys"].grad.numpy(), gold["g_means2d"], 1e-4, "g_means2d", frac_ok=0.995, rel_all=0.5)


@pytest.mark.gpu
def test_hip_matches_upstream_inria():
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    for i, gold in _cases(_load("upstream_inria.npz")):
        params, cam, wimg, bg = _inputs(gold["cfg"])
        m, s, q, o, c = [t.cuda().requires_grad_(True) for t in params]
        settings = ops.GaussianRasterizationSettings(
            image_height=cam["height"], image_width=cam["width"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=bg.cuda(), scale_modifier=1.0,
            viewmatrix=cam["world_to_camera"].cuda(), projmatrix=cam["full_projection"].cuda(), sh_degree=3, campos=cam["camera_center"].cuda())
        screen = torch.zeros_like(m, requires_grad=True)
        render, radii = ops.GaussianRasterizer(settings)(means3D=m, means2D=screen, opacities=o, shs=c, scales=s, rotations=q)
        (render * wimg.cuda()).sum().backward()
        _check(render.detach().cpu().numpy(), [t.grad.cpu().numpy() for t in (m, s, q, o, c)], gold, ("g_means", "g_scales", "g_quats", "g_opac", "g_shs"))
        assert_close_scaled(screen.grad.cpu().numpy(), gold["g_screen"], 1e-4, "g_screen", frac_ok=0.995, rel_all=0.5)


@pytest.mark.gpu
def test_hip_matches_upstream_gsplat():
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    for i, gold in _cases(_load("upstream_gsplat.npz")):
        params, cam, wimg, bg = _inputs(gold["cfg"])
        W, H = cam["width"], cam["height"]
        m, s, q, o, c = [t.cuda().requires_grad_(True) for t in params]
        vm = cam["world_to_camera"].T.contiguous().cuda()
        xys, depths, radii, conics, comp, tiles, _ = ops.project_gaussians(m, s, 1.0, q, vm[:3], cam["fx"], cam["fy"], cam["cx"], cam["cy"], H, W, 16)
        xys.retain_grad()
        rgbs = ops.sh_view_colors(3, m, cam["camera_center"].cuda(), c, None, radii > 0)
        img = ops.rasterize_gaussians(xys, depths, radii, conics, tiles, rgbs, o * comp[:, None], H, W, 16, bg.cuda(), absgrad=True, channels_first=True)
        (img * wimg.cuda()).sum().backward()
        _check(img.detach().cpu().numpy(), [t.grad.cpu().numpy() for t in (m, s, q, o, c)], gold, ("g_means", "g_scales", "g_quats", "g_opac", "g_shs"))
        assert_close_scaled(xys.grad.cpu().numpy(), gold["g_means2d"], 1e-4, "g_means2d", frac_ok=0.995, rel_all=0.5)
        assert_close_scaled(xys.absgrad.cpu().numpy(), gold["absgrad"], 1e-4, "absgrad", frac_ok=0.995, rel_all=0.5)

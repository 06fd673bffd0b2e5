"""The HIP surfel rasterizer at bench.py's metric size (S-1080p-1M): radii bit-exact, the forward on ~2k sampled pixels of 64 tiles
against the fp64 oracle, and a finite backward."""
import numpy as np
import pytest
import torch

import surfel_oracle as SO

pytestmark = pytest.mark.gpu

# colour, alpha and normal on unflagged pixels: test_surfel_gpu.TOL's sub-pixel surfels, at pixel coordinates up to 1920 instead of 96
TOL = 5e-5


def test_surfel_1080p_1m_sampled_pixels_and_finite_backward():
    import gspl_amd  # noqa: F401
    from gspl_amd import ops, synthetic
    dev = torch.device("cuda:0")
    wl = synthetic.WORKLOADS["S-1080p-1M"]
    W, H = wl["width"], wl["height"]
    means, scales, quats, opac, shs = synthetic.workload_scene(wl, seed=42)
    scales = scales[:, :2] * 2.0
    cam = synthetic.camera(W, H, wl["fx"])
    bg = torch.tensor([0.1, 0.2, 0.3])
    leaves = [t.to(dev).requires_grad_(True) for t in (means, scales, quats, opac, shs)]
    m, s, q, o, c = leaves
    screen = torch.zeros_like(m, requires_grad=True)
    st = ops.SurfelRasterizationSettings(H, W, cam["tanfovx"], cam["tanfovy"], bg.to(dev), 1.0, cam["world_to_camera"].to(dev),
                                         cam["full_projection"].to(dev), 3, cam["camera_center"].to(dev))
    color, radii, allmap = ops.SurfelGaussianRasterizer(st)(means3D=m, means2D=screen, opacities=o, shs=c, scales=s, rotations=q)
    (color.mean() + allmap[6].mean() + allmap[0].mean() * 1e-2).backward()
    torch.cuda.synchronize()
    for t in leaves + [screen]:
        assert bool(torch.isfinite(t.grad).all())
    assert float(m.grad.abs().sum()) > 0 and float(screen.grad[:, :2].abs().sum()) > 0
    # 64 tiles spread over the frame, 32 pixels in each
    g = np.random.default_rng(3)
    tw, th = (W + 15) // 16, (H + 15) // 16
    pick = np.zeros((H, W), dtype=bool)
    for t in g.choice(tw * th, size=64, replace=False):
        ty, tx = divmod(int(t), tw)
        ys = np.clip(ty * 16 + g.integers(0, 16, 32), 0, H - 1)
        xs = np.clip(tx * 16 + g.integers(0, 16, 32), 0, W - 1)
        pick[ys, xs] = True
    pix = torch.from_numpy(pick)
    with torch.no_grad():
        r = SO.render(means.double(), scales.double(), quats.double(), opac.double(), shs.double(), 3, cam["world_to_camera"].double(),
                      cam["full_projection"].double(), cam["camera_center"].double(), W, H, bg.double(), pixels=pix)
    fr = r["pre"]["radius_fragile"]
    assert int(fr.sum()) <= 2e-3 * fr.numel()          # extents within 1e-5 relative of an integer
    assert torch.equal(radii.cpu()[~fr], r["radii"][~fr]) and bool(((radii.cpu()[fr] - r["radii"][fr]).abs() <= 1).all())
    ok = pix & ~r["flagged"]
    assert int((pix & r["flagged"]).sum()) <= 0.01 * int(pix.sum())
    c64, a64 = color.detach().cpu().double(), allmap.detach().cpu().double()
    assert float((c64 - r["render"]).abs()[:, ok].max()) <= TOL
    for ch in (1, 2, 3, 4):
        assert float((a64[ch] - r["allmap"][ch]).abs()[ok].max()) <= TOL, ch
    for ch in (0, 5, 6):      # depth, median: their largest value; distortion: its terms' bound (w m^2 summed, m <= 1), the alpha
        scale = float(r["allmap"][1 if ch == 6 else ch][pix].abs().max()) + 1e-12
        assert float((a64[ch] - r["allmap"][ch]).abs()[ok].max()) <= 1e-5 * scale, ch

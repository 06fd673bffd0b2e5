"""The fused call's anti-aliasing and inverse-depth switches at the metric size and under adversarial memory: locked parity at
S-1080p-1M with both switches on, poisoned guard bands around every block of the call (the [N,4] rows, the 40 N-byte packed block, the
checkpoints with the 4th channel) with 0xFF / 0x00 pre-fills, the segmented backward carrying the 4th channel, and the densification
statistics inside the backward."""
import numpy as np
import pytest
import torch

from oracle import gsplat_oracle as O
import accel_oracle as A
from hip_helpers import check_guard_bands, cov2d_condition, cov_chain_slack, footprint_slack, guard_library_blocks

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 4096


def _settings(cam, W, H, bg):
    from gspl_amd import ops
    return ops.AccelRasterizationSettings(image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=bg.to(DEV),
                                          scale_modifier=1.0, viewmatrix=cam["world_to_camera"].to(DEV), projmatrix=cam["full_projection"].to(DEV),
                                          sh_degree=3, campos=cam["camera_center"].to(DEV), antialiasing=True)


def test_metric_point_S_1080p_1M_locked_both_switches():
    """The scene of test_locked_parity's metric point, both switches on: the oracle composites AT the kernel's per-splat values (means2d,
    conics, [N,4] colour | 1/z rows, effective opacities) over its lists; robust pixels within 1e-5 in all four channels, flagged pixels
    out of the loss on both sides, every gradient element within 1e-4 (|ref| + rms) plus the fp32 conditioning slack of the chain."""
    from gspl_amd import ops, synthetic
    wl = synthetic.WORKLOADS["S-1080p-1M"]
    W, H = wl["width"], wl["height"]
    params = O.synthetic_scene(wl["n"], seed=42)
    cam = O.synthetic_camera(W, H, wl["fx"])
    bg = torch.tensor([0.1, 0.2, 0.3])
    gen = torch.Generator().manual_seed(1)
    wimg, winv = torch.randn(3, H, W, generator=gen), torch.rand(1, H, W, generator=gen)
    ops.KEEP_LAST_RASTER = True
    try:
        leaves = [t.to(DEV).requires_grad_(True) for t in params]
        m, s, q, o, c = leaves
        img, radii, inv = ops.rasterize_inria_accel(_settings(cam, W, H, bg), m, torch.zeros_like(m, requires_grad=True), o, c, scales=s, rotations=q,
                                                    antialiasing=True, inverse_depth=True)
        last = ops.LAST_RASTER
        gpu_vals = [last[k].detach().cpu() for k in ("means2d", "conics", "colors", "opacities")]
        assert gpu_vals[2].shape == (wl["n"], 4)
        flat, offs = last["flatten_ids"].cpu().numpy(), last["offsets"].cpu().numpy()
        dl = [t.double().requires_grad_(True) for t in params]
        dm, ds, dq, do, dc = dl
        V = cam["world_to_camera"].double()
        xy, depths, r_radii, conics, mask = O.inria_preprocess(dm, ds, 1.0, dq, V, cam["full_projection"].double(), cam["tanfovx"], cam["tanfovy"], H, W)
        rgbs = torch.where(mask[:, None], O.sh_colors(3, dc, dm, cam["camera_center"].double(), detach_dirs=False), torch.zeros((), dtype=torch.float64))
        z = A.view_depth(dm, V)
        invd = torch.where(mask, 1.0 / torch.where(mask, z, torch.ones_like(z)), torch.zeros((), dtype=torch.float64))
        op = do.reshape(-1) * A.compensation(dm, ds, 1.0, dq, V, cam["tanfovx"], cam["tanfovy"], W, H)
        feats = torch.cat([rgbs, invd[:, None]], 1)
        bg4 = torch.cat([bg.double(), torch.zeros(1, dtype=torch.float64)])
        out, alpha, frag, locked = O.composite_locked(O.MODE_INRIA, (xy, conics, feats, op), gpu_vals, bg4, W, H, offs, flat, return_inputs=True)
        ref = out.permute(2, 0, 1)
        got = torch.cat([img, inv]).detach().cpu().double()
        d = (got - ref.detach()).abs().max(dim=0).values
        n_frag = int(frag.sum())
        assert n_frag <= 0.005 * frag.numel()
        assert float(d[~frag].max()) <= 1e-5, f"a robust pixel differs by {float(d[~frag].max()):.3e}"
        keepw = (~frag).double()
        (img * (wimg * keepw.float()).to(DEV)).sum().add_((inv * (winv * keepw.float()).to(DEV)).sum()).backward()
        ((ref[:3] * wimg.double() * keepw).sum() + (ref[3:] * winv.double() * keepw).sum()).backward()
        agree = ((radii > 0).cpu() == mask)
        assert int((~agree).sum()) <= max(1e-4 * agree.numel(), 2)
        keep = agree.numpy()
        kappa = cov2d_condition(conics.detach().numpy())[keep]
        extent = r_radii.numpy().astype(np.float64)[keep]
        failures = []
        for got_t, ref_t, name in zip(leaves, dl, ("means", "scales", "quats", "opacities", "shs")):
            g, rf = got_t.grad.cpu().double().numpy()[keep], ref_t.grad.numpy()[keep]
            rms = float(np.sqrt(np.mean(rf * rf))) + 1e-30
            allowed = 1e-4 * (np.abs(rf) + rms) + footprint_slack(rf, extent)
            if name in ("means", "scales", "quats", "opacities"):      # conic -> cov2D -> cov3D, and the compensation sqrt(det0 / det1)
                allowed = allowed + cov_chain_slack(rf, kappa)
            err = np.abs(g - rf)
            if (err > allowed).any():
                failures.append(f"{name}: {int((err > allowed).sum())} elements, worst ratio {float((err / allowed).max()):.2f}")
        assert not failures, "; ".join(failures)
    finally:
        ops.KEEP_LAST_RASTER = False


# (the segmentation is FIXED per case — off or "always" — so that the two pre-fills run the same code path: the adaptive mode may switch
# between the two forms from one frame to the next, and the segmented forward sums the colour per segment, a different rounding)
@pytest.mark.parametrize("workload,segmented", [("S-smoke-surfaces", "always"), ("S-smoke", False), ("S-1080p-1M-surfaces", "always")])
def test_guard_bands_and_prefills_with_both_switches(monkeypatch, workload, segmented):
    """Every block of the call (GSPL_BUF_GEOMETRY with the [N,4] rows, GSPL_BUF_PACKED of 40 N bytes, checkpoints with the 4th channel)
    between poisoned bands, the blocks themselves pre-filled with 0xFF (NaN, -1) and then 0x00: bands intact, images bit-equal."""
    from gspl_amd import ops, synthetic
    from gspl_amd.ops._state import STATE as S
    monkeypatch.setattr(S, "segmented_backward", segmented)
    wl = synthetic.WORKLOADS[workload]
    W, H = wl["width"], wl["height"]
    params = [t.to(DEV) for t in synthetic.workload_scene(wl, seed=42)]
    cams = synthetic.camera_set(W, H, wl["fx"], count=16, distance=wl.get("distance", 4.0))
    bg = torch.tensor([0.1, 0.2, 0.3])
    wimg = torch.randn(4, H, W, generator=torch.Generator().manual_seed(2)).to(DEV)
    images = {}
    for fill in (0xFF, 0x00):
        outers = guard_library_blocks(monkeypatch, GUARD, fill)
        images[fill] = []
        for k in (0, 0, 5):
            del outers[:]
            leaves = [t.detach().clone().requires_grad_(True) for t in params]
            m, s, q, o, c = leaves
            img, radii, inv = ops.rasterize_inria_accel(_settings(cams[k], W, H, bg), m, torch.zeros_like(m, requires_grad=True), o, c, scales=s,
                                                        rotations=q, antialiasing=True, inverse_depth=True)
            (torch.cat([img, inv]) * wimg).sum().backward()
            assert check_guard_bands(outers, f"{workload} view {k} fill {fill:#x}", GUARD) >= 4
            assert all(bool(torch.isfinite(t.grad).all()) for t in leaves)
            images[fill].append(torch.cat([img, inv]).detach())
    for a, b in zip(images[0xFF], images[0x00]):
        assert torch.equal(a, b)


def test_segmented_backward_carries_the_inverse_depth_channel(monkeypatch):
    """A trained-scene-shaped frame (heavy-tailed lists, needles) with checkpoints forced against the one-workgroup walk: two fp32
    summation orders of the same terms, which differ by the conditioning of the scene's needles.  The control is the three-channel frame
    (no inverse depth) under the same comparison: with the loss on the inverse depth ALONE, and on all four channels, the four-channel
    frame's disagreement must be of the control's size — a checkpoint that lost the 4th channel's accumulated sum would be off by O(1)."""
    from gspl_amd import ops, synthetic
    from gspl_amd.ops._state import STATE as S
    wl = synthetic.WORKLOADS["S-smoke-surfaces"]
    W, H = wl["width"], wl["height"]
    params = [t.to(DEV) for t in synthetic.workload_scene(wl, seed=42)]
    cam = O.synthetic_camera(W, H, wl["fx"])
    bg = torch.tensor([0.1, 0.2, 0.3])
    wimg = torch.randn(4, H, W, generator=torch.Generator().manual_seed(4)).to(DEV)
    only_inv = torch.zeros_like(wimg)
    only_inv[3] = wimg[3]

    def run(mode, invd, weights):
        monkeypatch.setattr(S, "segmented_backward", mode)
        ops.KEEP_LAST_RASTER = True
        try:
            leaves = [t.detach().clone().requires_grad_(True) for t in params]
            m, s, q, o, c = leaves
            img, radii, inv = ops.rasterize_inria_accel(_settings(cam, W, H, bg), m, torch.zeros_like(m, requires_grad=True), o, c, scales=s,
                                                        rotations=q, antialiasing=True, inverse_depth=invd)
            out = torch.cat([img, inv]) if invd else img
            (out * weights[:out.shape[0]]).sum().backward()
            torch.cuda.synchronize()
            segs = ops.LAST_RASTER["segment_count"]
            return out.detach(), [t.grad.clone() for t in leaves], None if segs is None else int(segs.item())
        finally:
            ops.KEEP_LAST_RASTER = False

    def disagreement(a, b):
        out = []
        for x, y in zip(a[1], b[1]):
            rms = float(y.double().pow(2).mean().sqrt()) + 1e-30
            out.append(float(((x - y).abs() / (y.abs() + rms)).max()))
        return np.array(out)

    control = disagreement(run(False, False, wimg), run("always", False, wimg))
    for weights, what in ((only_inv, "inverse depth only"), (wimg, "all four channels")):
        plain, seg = run(False, True, weights), run("always", True, weights)
        assert plain[2] is None and seg[2] is not None and seg[2] > 0, "the forced frame published no segments"
        # (the segmented forward sums the colour per segment and then the segments: the same terms, another rounding)
        assert float((plain[0] - seg[0]).abs().max()) <= 1e-5
        d = disagreement(plain, seg)
        print(f"[segmented, {what}] worst element / (|g| + rms) per parameter {d}, three-channel control {control}")
        # opacities and SH: the compositing's own per-splat sums, in which a wrong "behind" sum at a segment start (the checkpoint's
        # accumulated colour, 4th channel included) enters v_alpha directly — tight.  Means / scales / rotations pass the conic's gradient
        # through conic -> cov2D -> cov3D, which amplifies the summation-order difference by the needles' conditioning (hip_helpers.
        # cov_chain_slack: kappa ~ 4000 in this scene) and by the size of the loss: bounded against the control, loosely.
        assert (d[3:] <= 1e-4).all(), (what, d)
        assert (d[:3] <= np.maximum(20.0 * control[:3], 2e-3)).all(), (what, d, control)


def test_densification_statistics_in_the_backward_with_both_switches():
    """ABI 34's statistics inside the backward (density.request_stats_in_backward) on a frame with both switches: the same values as
    `update_densification_stats` after the backward from the screen-space gradient."""
    from gspl_amd import density, ops, synthetic
    wl = synthetic.WORKLOADS["S-smoke"]
    W, H = wl["width"], wl["height"]
    means, scales, quats, opac, shs = O.synthetic_scene(wl["n"], seed=42)
    cam = O.synthetic_camera(W, H, wl["fx"])
    bg = torch.tensor([0.1, 0.2, 0.3])
    N = means.shape[0]
    results = []
    for in_backward in (False, True):
        leaves = [t.to(DEV).requires_grad_(True) for t in (means, scales * 4, quats, opac, shs)]
        m, s, q, o, c = leaves
        screen = torch.zeros_like(m, requires_grad=True)
        accum, denom, maxr = torch.zeros(N, 1, device=DEV), torch.zeros(N, 1, device=DEV), torch.zeros(N, device=DEV)
        img, radii, inv = ops.rasterize_inria_accel(_settings(cam, W, H, bg), m, screen, o, c, scales=s, rotations=q, antialiasing=True, inverse_depth=True)
        req = density.request_stats_in_backward(radii, accum, denom, maxr) if in_backward else None
        ((img - 0.4).abs().mean() + (inv - 0.1).abs().mean()).backward()
        if in_backward:
            assert req is not None and req.applied
        else:
            vis = radii > 0
            accum[vis] += torch.norm(screen.grad[vis, :2], dim=-1, keepdim=True)
            denom[vis] += 1
            maxr[vis] = torch.maximum(maxr[vis], radii[vis].float())
        results.append((accum, denom, maxr))
    for a, b in zip(*results):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)

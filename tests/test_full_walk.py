"""Compositing after an opacity reset: every splat just above the 1/255 skip, no pixel saturating, every pixel walking its whole list.

The vanilla, 2DGS and Taming density controllers reset every opacity to min(o, 0.01) every 3000 steps.  For the next few hundred steps
the transmittance stop never fires, and the backward rebuilds T over the whole walk as T *= 1 / (1 - a), compounded over every entry
it takes, where the fp64 oracle divides.  Here:

  * a deep column: ~1500 splats of alpha ~0.0046 over every pixel of the tiles (final T ~1e-3), compositing backward against the fp64
    oracle, every element within 1e-4 of |ref| + rms;
  * a walk of more than SEG_MAX * SEG entries in one tile (csrc/gspl_composite.h): the segmented backward of the fused Inria call cuts
    it into SEG_MAX segments and the last one takes the remainder; against the plain walk and against the fp64 oracle.
"""
import numpy as np
import pytest
import torch

from oracle import gsplat_oracle as O
from hip_helpers import assert_close_scaled, hip_composite_bwd, hip_composite_fwd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEG, SEG_MAX = 256, 255      # csrc/gspl_composite.h


def _deep_column(mode, D, n=1500, W=32, H=32, seed=3):
    """n large splats over a W x H image (tile 16): alpha ~0.0042-0.005 at every pixel, final T ~1e-3."""
    g = torch.Generator().manual_seed(seed)
    centre = torch.tensor([W / 2.0, H / 2.0]) - (0.0 if mode == O.MODE_GSPLAT else 0.5)
    xy = (centre + (torch.rand(n, 2, generator=g) - 0.5) * 8).float()
    s_major = torch.rand(n, generator=g) * 150 + 150
    s_minor = s_major * (torch.rand(n, generator=g) * 0.5 + 0.5)
    th = torch.rand(n, generator=g) * 3.14159
    cx, sx = torch.cos(th), torch.sin(th)
    cov_a = cx * cx * s_major ** 2 + sx * sx * s_minor ** 2
    cov_b = cx * sx * (s_major ** 2 - s_minor ** 2)
    cov_c = sx * sx * s_major ** 2 + cx * cx * s_minor ** 2
    det = cov_a * cov_c - cov_b * cov_b
    conics = torch.stack([cov_c / det, -cov_b / det, cov_a / det], 1).float()
    radii = torch.full((n,), 64, dtype=torch.int32)
    depths = torch.rand(n, generator=g) * 8 + 0.2
    opac = (torch.rand(n, generator=g) * 0.0006 + 0.0044).float()
    colors = torch.rand(n, D, generator=g)
    bg = torch.rand(D, generator=g)
    _, _, flat, offs = O.isect_tiles(mode, xy, radii, depths, W, H)
    return xy, conics, colors, opac, bg, flat, offs


@pytest.mark.parametrize("mode", [O.MODE_GSPLAT, O.MODE_INRIA])
@pytest.mark.parametrize("D", [3, 4])
def test_deep_unsaturated_column_against_the_oracle(mode, D):
    import gspl_amd  # noqa: F401
    W, H = 32, 32
    xy, conics, colors, opac, bg, flat, offs = _deep_column(mode, D, W=W, H=H)
    out_ref, alpha_ref, last_ref, frag = O.composite_fwd(mode, xy, conics, colors, opac, bg, W, H, offs, flat)
    c = lambda a: torch.as_tensor(a).contiguous().to(DEV)
    out, alphas, final_T, last = hip_composite_fwd(mode, c(xy), c(conics), c(colors), c(opac), c(bg), W, H, c(offs), c(flat))
    T = final_T.cpu().numpy()
    # (the oracle flags the pixels whose centre lies within ~0.1 px of a mean, where the sign test on sigma ~ 0 is a decision: they
    # carry no loss on either side, as in test_hip_parity.test_composite_fwd_bwd_vs_oracle; 34 of the 1024 pixels in this scene)
    ok = frag == 0
    print(f"[deep column] mode={mode} D={D}: {len(flat)} entries, final T {T.min():.2e} .. {T.max():.2e}, {int((~ok).sum())} pixels flagged")
    assert ok.mean() > 0.95
    assert 2e-4 < T.min() and T.max() < 5e-3, "not a deep unsaturated column"
    assert np.array_equal(last.cpu().numpy()[ok], last_ref[ok])
    assert np.abs(out.cpu().numpy() - out_ref)[ok].max() <= 1e-5
    assert np.abs(final_T.cpu().numpy() - (1.0 - alpha_ref))[ok].max() <= 1e-5

    gv = torch.Generator().manual_seed(4)
    v_out, v_alpha = torch.randn(H, W, D, generator=gv), torch.randn(H, W, generator=gv)
    v_out[torch.from_numpy(~ok)] = 0.0
    v_alpha[torch.from_numpy(~ok)] = 0.0
    got = hip_composite_bwd(mode, c(xy), c(conics), c(colors), c(opac), c(bg), W, H, c(offs), c(flat), final_T, last, c(v_out), c(v_alpha),
                            absgrad=True)
    ref = O.composite_bwd(mode, xy, conics, colors, opac, bg, W, H, offs, flat, 1.0 - final_T.cpu().double().numpy(), last.cpu().numpy(),
                          v_out.double().numpy(), v_alpha.double().numpy(), fragile_px=frag, absgrad=True)
    for k in ("v_means2d", "v_means2d_abs", "v_conics", "v_colors", "v_opacities"):
        g, r = got[k].cpu().numpy().astype(np.float64), ref[k]
        worst = float((np.abs(g - r) / (np.abs(r) + np.sqrt(np.mean(r * r)))).max())
        print(f"[deep column] {k}: worst element / (|ref| + rms) {worst:.3e}")
        assert_close_scaled(g, r, 1e-4, f"{k} mode={mode} D={D}", frac_ok=1.0)


def _long_tile_scene(n=70000, W=64, H=64, seed=8):
    """n tiny splats (opacity 0.005-0.01) with their means inside tile (0, 0) of a W x H frame: one walk of n > SEG_MAX * SEG entries,
    each pixel blending a few hundred of them, unsaturated.  (The Inria preprocess adds 0.3 px^2 to every 2D covariance, so a
    footprint cannot shrink below that: the opacities are lower than the reset value to keep the column from saturating.)"""
    from gspl_amd import synthetic
    cam = synthetic.camera(W, H, 80.0)
    g = torch.Generator().manual_seed(seed)
    zc = torch.rand(n, generator=g) * 2 + 3
    pix = torch.rand(n, 2, generator=g) * 13 + 1           # Inria pixel centres 0..15 lie in tile (0, 0); no reach into its neighbours
    ndc = (2 * pix.double() + 1) / torch.tensor([W, H], dtype=torch.float64) - 1
    tan = torch.tensor([cam["tanfovx"], cam["tanfovy"]], dtype=torch.float64)
    means = torch.cat([ndc * tan * zc[:, None].double(), (zc - 4.0)[:, None].double()], 1).float()
    scales = (torch.rand(n, 3, generator=g) * 0.2 + 0.1) * zc[:, None] / 80.0
    quats = torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=1)
    opac = (torch.rand(n, 1, generator=g) * 0.005 + 0.005).float()
    shs = torch.randn(n, 16, 3, generator=g) * 0.2
    return (means, scales.float(), quats, opac, shs), cam


def test_a_walk_of_more_than_seg_max_segments():
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    from test_segmented_backward import _render, _close
    from test_locked_parity import _run_locked
    params, cam = _long_tile_scene()
    W, H = cam["width"], cam["height"]
    img_s, radii_s, grads_s, count, longest, _ = _render(params, cam, True)
    packed_s = _render.packed
    img_p, radii_p, grads_p, count_p, longest_p, _ = _render(params, cam, False)
    packed_p = _render.packed
    print(f"[long walk] longest walk {longest}, segments published {count}")
    assert longest > SEG_MAX * SEG and longest == longest_p
    assert count_p is None
    # one tile of more than SEG_MAX segments: SEG_MAX - 1 published beyond its first, the last taking the remainder
    assert count == SEG_MAX - 1, count
    assert torch.equal(radii_s, radii_p) and float((img_s - img_p).abs().max()) <= 2e-6
    for lo, hi, name in ((0, 2, "dL/dmeans2d"), (2, 5, "dL/dconic"), (5, 6, "dL/dopacity"), (6, 9, "dL/dcolour")):
        _close(packed_s[:, lo:hi], packed_p[:, lo:hi], "compositing " + name)
    for a, b, name in zip(grads_s, grads_p, ("means", "scales", "quats", "opacities", "shs", "viewspace_points.grad")):
        _close(a, b, name)
    wimg = torch.randn(3, H, W, generator=torch.Generator().manual_seed(6))
    prev = ops.SEGMENTED_BACKWARD
    for seg in ("always", False):
        ops.SEGMENTED_BACKWARD = seg
        try:
            _run_locked("vanilla", params, cam, W, H, 3, torch.tensor([0.1, 0.2, 0.3]), wimg)
        finally:
            ops.SEGMENTED_BACKWARD = prev

"""fp64 oracle of the Taming-3DGS rasterizer (`diff_accel_gaussian_rasterization`): the vanilla pipeline of oracle/gsplat_oracle.py with
the two switches of the fused Inria call, composed from the functions that module exports.

  anti-aliasing (GSPL_INRIA_ANTIALIAS): det0 / det1 = determinant of the EWA 2D covariance before / after the +0.3 dilation,
      comp = sqrt(max(2.5e-5, det0 / det1)), composited opacity = opacity * comp (graphdeco `dr_aa`, restated);
  inverse depth (GSPL_INRIA_INVDEPTH): a 4th composited channel 1 / z of the view-space depth, background 0 — z NOT detached
      (`inria_preprocess` detaches the depth it returns: it only orders the lists there).
Gradients come from autograd through these expressions and the C oracle's analytic compositing backward (`composite_c`)."""
import torch

from oracle import gsplat_oracle as O


def _cov3d(scales, scale_modifier, quats, cov3d_precomp):
    if cov3d_precomp is None:
        return O.cov3d_from_scale_rot(scales, scale_modifier, quats)
    s = cov3d_precomp
    return torch.stack([s[:, 0], s[:, 1], s[:, 2], s[:, 1], s[:, 3], s[:, 4], s[:, 2], s[:, 4], s[:, 5]], dim=-1).reshape(-1, 3, 3)


def compensation(means, scales, scale_modifier, quats, viewmatrix, tanfovx, tanfovy, width, height, cov3d_precomp=None, front=None):
    """comp [N] = sqrt(max(2.5e-5, det0 / det1)) of the Inria preprocess's 2D covariance; rows behind the near plane get 1."""
    dt = means.dtype
    V = viewmatrix.to(dt)
    pv = means @ V[:3, :3] + V[3, :3]
    if front is None:
        front = pv[:, 2].detach() > 0.2
    pv_safe = torch.where(front[:, None], pv, torch.ones_like(pv))
    fx, fy = width / (2.0 * tanfovx), height / (2.0 * tanfovy)
    cov2d = O.ewa_cov2d(pv_safe, _cov3d(scales, scale_modifier, quats, cov3d_precomp), V[:3, :3].T, fx, fy, 1.3 * tanfovx, 1.3 * tanfovy,
                        inria_clamp_grad=True)
    a0, b, c0 = cov2d[:, 0, 0], cov2d[:, 0, 1], cov2d[:, 1, 1]
    det0 = a0 * c0 - b * b
    det1 = (a0 + 0.3) * (c0 + 0.3) - b * b
    comp = torch.sqrt(torch.clamp_min(det0 / det1, 2.5e-5))
    return torch.where(front, comp, torch.ones((), dtype=dt))


def view_depth(means, viewmatrix):
    """z of the view-space mean, differentiable (the inverse-depth channel's chain into the means)."""
    V = viewmatrix.to(means.dtype)
    return means @ V[:3, 2] + V[3, 2]


def render_inria_accel(means, scales, quats, opacities, sh_coeffs, degree, viewmatrix, projmatrix, camera_center, tanfovx, tanfovy,
                       width, height, background, antialias=False, scale_modifier=1.0, colors_precomp=None, cov3d_precomp=None):
    """Returns dict(render [3,H,W], inverse_depth [1,H,W], radii, opacities (effective), xy, conics, depths, offsets, flatten_ids, ...)."""
    xy, depths, radii, conics, mask = O.inria_preprocess(means, scales, scale_modifier, quats, viewmatrix, projmatrix, tanfovx, tanfovy,
                                                         height, width, cov3d_precomp=cov3d_precomp)
    zf = torch.zeros((), dtype=means.dtype)
    if colors_precomp is None:
        rgbs = O.sh_colors(degree, sh_coeffs, means, camera_center, detach_dirs=False)
    else:
        rgbs = colors_precomp
    rgbs = torch.where(mask[:, None], rgbs, zf)
    z = view_depth(means, viewmatrix)
    invd = torch.where(mask, 1.0 / torch.where(mask, z, torch.ones_like(z)), zf)
    op = opacities.reshape(-1)
    if antialias:
        op = op * compensation(means, scales, scale_modifier, quats, viewmatrix, tanfovx, tanfovy, width, height, cov3d_precomp)
    tiles, ids, flat, offs = O.isect_tiles(O.MODE_INRIA, xy, radii, depths, width, height)
    bg4 = torch.cat([background.reshape(-1).to(means.dtype), torch.zeros(1, dtype=means.dtype)])
    feats = torch.cat([rgbs, invd[:, None]], dim=1)
    out, alpha = O.composite_c(O.MODE_INRIA, xy, conics, feats, op, bg4, width, height, offs, flat)
    img = out.permute(2, 0, 1)
    return {"render": img[:3], "inverse_depth": img[3:], "alpha": alpha, "xy": xy, "radii": radii, "mask": mask, "depths": depths,
            "conics": conics, "rgbs": rgbs, "features": feats, "opacities": op, "flatten_ids": flat, "offsets": offs}

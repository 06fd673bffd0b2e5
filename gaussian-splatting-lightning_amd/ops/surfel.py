"""The 2D Gaussian Splatting (surfel) rasterizer: `SurfelRasterizationSettings`, `SurfelGaussianRasterizer` — the interface of
`diff_surfel_rasterization` (reference call site internal/renderers/vanilla_2dgs_renderer.py:50-90), one C-ABI call per direction
(`gspl_rasterize_surfel_fwd/bwd`, csrc/surfel.hip).

forward(...) returns (color [3,H,W], radii [N] i32, allmap [7,H,W]); allmap = depth | alpha | view-space normal (3) | median depth |
distortion.  `means2D.grad` receives upstream's densification proxy (include/gspl_hip.h section 6c), not a true derivative."""
from __future__ import annotations

import ctypes

import torch

from .. import _lib as L
from ._common import _guarded, _f32c, _grad_or_zeros
from ._frame import FrameBlocks
from .inria import GaussianRasterizationSettings as SurfelRasterizationSettings, _check_inputs      # (upstream's 12 fields, the same tuple)


class _SurfelRasterizeFn(torch.autograd.Function):
    @staticmethod
    @_guarded(1)
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, settings):
        s: SurfelRasterizationSettings = settings
        dev = means3D.device
        means3D, sh, colors_precomp, scales, rotations = map(_f32c, (means3D, sh, colors_precomp, scales, rotations))
        N = means3D.shape[0]
        H, W = int(s.image_height), int(s.image_width)
        opac = _f32c(opacities).reshape(-1)
        viewm, projm, campos = _f32c(s.viewmatrix.to(dev)), _f32c(s.projmatrix.to(dev)), _f32c(s.campos.to(dev))
        bg = _f32c(s.bg.to(dev)).reshape(-1)
        if bg.numel() != 3:
            raise ValueError(f"bg must hold 3 values, got {bg.numel()}")
        if N > 0 and (scales.dim() != 2 or scales.shape[1] != 2 or rotations.shape != (N, 4) or opac.shape[0] != N):
            raise ValueError(f"scales must be [N,2], rotations [N,4], opacities [N] or [N,1]; got {tuple(scales.shape)}, "
                             f"{tuple(rotations.shape)}, {tuple(opacities.shape)}")
        if colors_precomp is None and sh is None:
            raise ValueError("either shs or colors_precomp")
        if colors_precomp is not None and sh is not None:
            raise ValueError("shs and colors_precomp are exclusive")
        n_coeffs = 0 if sh is None else sh.shape[1]
        radii = torch.empty((N,), dtype=torch.int32, device=dev)
        out = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        allmap = torch.empty((7, H, W), dtype=torch.float32, device=dev)
        state = L.SurfelState()
        with FrameBlocks(dev) as frame:
            L.call("gspl_rasterize_surfel_fwd", N, int(s.sh_degree), n_coeffs, L.ptr(means3D), L.ptr(scales), L.ptr(rotations), L.ptr(sh),
                   L.ptr(colors_precomp), L.ptr(opac), L.ptr(viewm), L.ptr(projm), L.ptr(campos), L.ptr(bg), W, H, float(s.scale_modifier),
                   frame.callback, None, L.ptr(out), L.ptr(allmap), L.ptr(radii), ctypes.byref(state), L.stream())
        ctx.save_for_backward(means3D, scales, rotations, sh, viewm, projm, campos, bg, radii, *frame.saved())
        ctx.state, ctx.frame = state, frame
        ctx.cfg = (int(s.sh_degree), n_coeffs, float(s.scale_modifier), colors_precomp is not None, opacities.shape, scales.shape)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(radii)
        return out, radii, allmap

    @staticmethod
    @_guarded(0)
    def backward(ctx, v_out, _v_radii, v_allmap):
        means3D, scales, rotations, sh, viewm, projm, campos, bg, radii, *saved_blocks = ctx.saved_tensors
        ctx.frame.unpack(saved_blocks)      # (the state points into them: they must not have moved)
        degree, n_coeffs, scale_modifier, has_precomp, opac_shape, scales_shape = ctx.cfg
        st = ctx.state
        N, H, W = st.N, st.height, st.width
        dev = means3D.device
        v_out = _grad_or_zeros(v_out, (3, H, W), dev)
        v_allmap = _grad_or_zeros(v_allmap, (7, H, W), dev)
        v_rows = torch.empty((N, 18), dtype=torch.float32, device=dev)
        v_means = torch.empty((N, 3), dtype=torch.float32, device=dev)
        v_means2d = torch.empty((N, 3), dtype=torch.float32, device=dev)
        v_scales = torch.empty((N, 2), dtype=torch.float32, device=dev)
        v_rot = torch.empty((N, 4), dtype=torch.float32, device=dev)
        v_opac = torch.empty((N,), dtype=torch.float32, device=dev)
        v_sh = None if has_precomp else torch.empty_like(sh)
        v_cp = torch.empty((N, 3), dtype=torch.float32, device=dev) if has_precomp else None
        if N > 0:
            with FrameBlocks(dev) as scratch:      # (the deterministic mode's per-entry rows: scratch of this call)
                L.call("gspl_rasterize_surfel_bwd", degree, n_coeffs, L.ptr(means3D), L.ptr(scales), L.ptr(rotations), L.ptr(sh), L.ptr(viewm),
                       L.ptr(projm), L.ptr(campos), L.ptr(bg), scale_modifier, L.ptr(radii), ctypes.byref(st), L.ptr(v_out), L.ptr(v_allmap),
                       scratch.callback, None, L.ptr(v_rows), L.ptr(v_means), L.ptr(v_means2d), L.ptr(v_sh), L.ptr(v_cp), L.ptr(v_opac),
                       L.ptr(v_scales), L.ptr(v_rot), L.stream())
        # order: means3D, means2D, sh, colors_precomp, opacities, scales, rotations, settings
        return v_means, v_means2d, v_sh, v_cp, v_opac.reshape(opac_shape), v_scales.reshape(scales_shape), v_rot, None


def rasterize_surfels(settings: SurfelRasterizationSettings, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                      rotations=None):
    """(color [3,H,W], radii [N], allmap [7,H,W]) of the surfels; the op `SurfelGaussianRasterizer` calls (tests swap it)."""
    return _SurfelRasterizeFn.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, settings)


class SurfelGaussianRasterizer(torch.nn.Module):
    """`diff_surfel_rasterization.GaussianRasterizer` on the HIP kernels."""

    def __init__(self, raster_settings: SurfelRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
        _check_inputs(shs, colors_precomp)
        if cov3D_precomp is not None:
            raise NotImplementedError("precomputed transforms (cov3D_precomp) are not supported by the HIP surfel rasterizer; pass scales "
                                      "and rotations")
        if scales is None or rotations is None:
            raise Exception("Please provide scales and rotations")
        from . import surfel as _self      # late binding: the op can be replaced (tests) after import
        return _self.rasterize_surfels(self.raster_settings, means3D, means2D, opacities, shs=shs, colors_precomp=colors_precomp,
                                       scales=scales, rotations=rotations)

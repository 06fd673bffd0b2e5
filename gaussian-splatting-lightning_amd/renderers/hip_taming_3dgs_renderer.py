"""HipTaming3DGSRenderer — drop-in for the reference's `Taming3DGSRenderer` (internal/renderers/taming_3dgs_renderer.py:8-117), backed by
the fused HIP Inria call of ops/inria.py with its two switches (GSPL_INRIA_ANTIALIAS, GSPL_INRIA_INVDEPTH) instead of
`diff_accel_gaussian_rasterization`.

Select with   --model.renderer gspl_amd.renderers.HipTaming3DGSRenderer   (`--model.renderer.anti_aliased true` for
the `-aa` configurations).  Outputs (taming_3dgs_renderer.py:105-117): `render` [3,H,W], `inverse_depth` [1,H,W] (composited 1 / z,
background 0; only when `render_types` asks for "inverse_depth" — otherwise None and the three-channel compositing runs),
`viewspace_points` (its `.grad[:, :2]` receives the NDC-scaled screen-space gradient), `visibility_filter`, `radii`.
"""
from __future__ import annotations

from typing import Dict

import torch

from .. import ops
from .renderer import (Renderer, RendererOutputInfo, RendererOutputTypes, model_sh_pair, model_geometry, raster_settings, screenspace_carrier,
                       marked_visibility)


class HipTaming3DGSRenderer(Renderer):
    def __init__(self, anti_aliased: bool = False, filter_2d_kernel_size: float = 0.3, fuse_activations: bool = True):
        """anti_aliased: the Mip-Splatting 2D filter (`antialiasing=True`); its dilation is the rasterizer's fixed 0.3, as the reference
        asserts.  fuse_activations: as `HipVanillaRenderer`'s (the model's raw parameters, activations inside the kernels)."""
        super().__init__()
        if anti_aliased:
            assert filter_2d_kernel_size == 0.3
        self.anti_aliased = anti_aliased
        self.filter_2d_kernel_size = filter_2d_kernel_size
        self.fuse_activations = fuse_activations

    def forward(self, viewpoint_camera, pc, bg_color: torch.Tensor, scaling_modifier=1.0, render_types: list = None, **kwargs):
        if render_types is None:
            render_types = ["rgb"]
        want_invdepth = "inverse_depth" in render_types
        means3D = pc.get_xyz
        screenspace_points = screenspace_carrier(means3D, bg_color.device)
        settings = raster_settings(viewpoint_camera, bg_color, scaling_modifier, pc.active_sh_degree)
        scales, rotations, opacities, raw = model_geometry(pc, self.fuse_activations)

        shs = shs_rest = None
        colors_precomp = kwargs.get("colors_precomp", None)
        if colors_precomp is None:
            shs, shs_rest = model_sh_pair(pc)

        rendered_image, radii, inverse_depth = ops.rasterize_inria_accel(
            settings, means3D, screenspace_points, opacities, shs, colors_precomp, scales, rotations, None, shs_rest=shs_rest,
            raw_parameters=raw, antialiasing=self.anti_aliased, inverse_depth=want_invdepth)
        return {
            "render": rendered_image,
            "inverse_depth": inverse_depth,
            "viewspace_points": screenspace_points,
            "visibility_filter": marked_visibility(radii),
            "radii": radii,
        }

    def get_available_outputs(self) -> Dict:
        return {"rgb": RendererOutputInfo("render"), "inverse_depth": RendererOutputInfo("inverse_depth", RendererOutputTypes.GRAY)}

"""HipGSplatContrastiveFeatureRenderer — drop-in for the reference's `GSplatContrastiveFeatureRenderer`
(internal/renderers/gsplat_contrastive_feature_renderer.py; the renderer of SegAnyGS, internal/segany_splatting.py:52,
configs/segany_splatting.yaml) on the HIP ops: `forward(..., semantic_features=...)` composites one 32-wide feature row per Gaussian
of a frozen model, optionally at a reduced resolution (`feature_map_width`), and `depth_forward` an accumulated depth map.

Both go through `ops.rasterize_features`: one launch over all channels and a backward that computes the feature gradient alone.
Should the model's geometry require a gradient, that op serves the call with the general compositing path, as the reference's
`rasterize_gaussians` would.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from .. import ops
from .renderer import Renderer, camera_scalars
from .hip_gsplat_renderer import DEFAULT_ANTI_ALIASED_STATUS, DEFAULT_BLOCK_SIZE, _project


class HipGSplatContrastiveFeatureRenderer(Renderer):
    def __init__(self, feature_map_width: int = -1) -> None:
        super().__init__()
        self.block_size = DEFAULT_BLOCK_SIZE
        self.anti_aliased = DEFAULT_ANTI_ALIASED_STATUS
        self.feature_map_width = feature_map_width

    def _project(self, viewpoint_camera, pc, scaling_modifier, width: int = -1):
        """Projection at the camera's resolution, or at `width` pixels across with the intrinsics scaled to match."""
        W, H, fx, fy, cx, cy = camera_scalars(viewpoint_camera, ("width", "height", "fx", "fy", "cx", "cy"))
        W, H = int(W), int(H)
        camera = viewpoint_camera
        if width > 0:
            height = int(width * H / W)
            x_scale, y_scale = width / W, height / H
            # same pose, scaled intrinsics; the pose's cached device matrix travels with it
            camera = SimpleNamespace(world_to_camera=viewpoint_camera.world_to_camera, fx=fx * x_scale, fy=fy * y_scale,
                                     cx=cx * x_scale, cy=cy * y_scale,
                                     _gspl_viewmat=getattr(viewpoint_camera, "_gspl_viewmat", None))
            W, H = width, height
        projected = _project(pc.get_xyz, pc.get_scaling, pc.get_rotation, camera, scaling_modifier, self.block_size, W, H)
        if camera is not viewpoint_camera:
            try:
                viewpoint_camera._gspl_viewmat = camera._gspl_viewmat
            except Exception:      # a frozen camera type: no cache
                pass
        opacities = pc.get_opacity
        if self.anti_aliased is True:
            opacities = opacities * projected[4][:, None]
        return projected, opacities, W, H

    def forward(self, viewpoint_camera, pc, bg_color: torch.Tensor, scaling_modifier=1.0, semantic_features: torch.Tensor = None, **kwargs):
        (xys, depths, radii, conics, comp, num_tiles_hit, _), opacities, W, H = self._project(
            viewpoint_camera, pc, scaling_modifier, self.feature_map_width)
        # [D,H,W] straight from the kernel (the reference permutes an [H,W,D] image)
        features = ops.rasterize_features(xys, depths, radii, conics, num_tiles_hit, semantic_features, opacities, H, W, self.block_size,
                                          background=bg_color, channels_first=True)
        return {
            "render": features,
            "viewspace_points": xys,
            "viewspace_points_grad_scale": 0.5 * max(H, W),
            "visibility_filter": radii > 0,
            "radii": radii,
        }

    def depth_forward(self, viewpoint_camera, pc):
        (xys, depths, radii, conics, comp, num_tiles_hit, _), opacities, W, H = self._project(viewpoint_camera, pc, 1.)
        return ops.rasterize_features(xys, depths, radii, conics, num_tiles_hit, depths.unsqueeze(-1), opacities, H, W, self.block_size,
                                      background=None, channels_first=True)      # (a zero background)

"""HipGlossyRenderer — drop-in for the reference's `GlossyRenderer` (internal/renderers/glossy_renderer.py; configs/glossy.yaml):
the staged gsplat-v1 renderer with a VIEW-DEPENDENT opacity, a one-channel spherical-harmonics expansion (`opacities` [N, 1, 1] +
`opacity_rest` [N, Kr, 1] of internal/models/glossy_gaussian.py) evaluated every step at the normalised view direction, + 0.5,
clamped to [0, 1].

Select with   --config configs/glossy.yaml --model.renderer gspl_amd.renderers.HipGlossyRenderer   (INTEGRATION.md).

The reference evaluates the expansion with F.normalize + `eval_sh_decomposed` + clamp in torch ops on [N, 1] tensors; here it is ONE
`ops.sh_view_opacities` launch (one more in the backward) that reads both parameters in place.  All N rows are evaluated, as in the
reference: its density controller's `update_opacity_max(outputs["opacities"])` reads the invisible rows too.  The colours are the
inherited `get_rgbs`, which already is the reference's clamp(SH + 0.5, min=0).  The reference's `GlossyGaussianModel` and its
`VanillaDensityController(cull_by_max_opacity=True)` are used unedited.

Not built: half precision, a fused running maximum for `opacity_max`, the distributed renderer, colour and opacity in one launch."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Tuple

from .. import ops
from .hip_gsplat_v1_renderer import HipGSplatV1Renderer, HipGSplatV1RendererModule


@dataclass
class HipGlossyRenderer(HipGSplatV1Renderer):
    def instantiate(self, *args, **kwargs) -> "HipGlossyRendererModule":
        return HipGlossyRendererModule(self)


class HipGlossyRendererModule(HipGSplatV1RendererModule):
    def get_opacities(self, camera, gaussian_model, projections: Tuple, visibility_filter, status: Any, **kwargs):
        properties = getattr(gaussian_model, "properties", {})
        if "opacity_rest" not in properties:
            raise TypeError(f"HipGlossyRenderer needs a model with an `opacity_rest` property (the reference's GlossyGaussian, "
                            f"internal/models/glossy_gaussian.py); {type(gaussian_model).__name__} has {sorted(properties)}")
        opacities = ops.sh_view_opacities(gaussian_model.active_sh_degree, gaussian_model.get_xyz, camera.camera_center,
                                          properties["opacities"], properties["opacity_rest"])
        return opacities, status

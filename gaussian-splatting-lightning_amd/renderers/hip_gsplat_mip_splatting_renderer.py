"""HipGSplatMipSplattingRendererV2 and HipGSplatAppearanceEmbeddingMipRenderer — drop-ins for the reference's
`GSplatMipSplattingRendererV2` (internal/renderers/gsplat_mip_splatting_renderer_v2.py; configs/mip_splatting_gsplat_v2*.yaml) and
`GSplatAppearanceEmbeddingMipRenderer` (internal/renderers/gsplat_appearance_embedding_renderer.py:326-361): the staged gsplat-v1
renderer, and the appearance-embedding renderer, on a model that carries a Mip-Splatting 3D filter.

Select with   --model.gaussian gspl_amd.mip.HipMipSplatting --model.renderer gspl_amd.renderers.HipGSplatMipSplattingRendererV2
(INTEGRATION.md); the reference's own `MipSplatting` model works as well.

The 2D filter is the projection's `filter_2d_kernel_size = 0.1` with `anti_aliased`.  The 3D filter is applied to the scales, and its
compensation to the opacities, every step: in the reference a dozen elementwise torch launches on the activated getters (ten more
launches), here ONE `ops.mip_apply_3d_filter` launch (one more in the backward) that reads the model's raw parameters in place when
its activations are the vanilla model's (gspl_amd.mip.filtered_scales_and_opacities).  With the reference's `MipSplattingModel` the
plugin still takes that fused call: the model's own torch method is not used.

Not built: the old `MipSplattingGSplatRenderer`, the distributed appearance-Mip renderer, half precision."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Tuple

from .. import mip as _mip
from .hip_gsplat_v1_renderer import HipGSplatV1Renderer, HipGSplatV1RendererModule
from .hip_gsplat_appearance_embedding_renderer import HipGSplatAppearanceEmbeddingRenderer, HipGSplatAppearanceEmbeddingRendererModule


@dataclass
class HipGSplatMipSplattingRendererV2(HipGSplatV1Renderer):
    filter_2d_kernel_size: float = 0.1

    def instantiate(self, *args, **kwargs) -> "HipGSplatMipSplattingRendererV2Module":
        return HipGSplatMipSplattingRendererV2Module(self)


class HipMipSplattingRendererMixin:
    """The reference mixin's contract: `get_scales` -> (filtered scales, the compensated opacities as `status`), `get_opacities` ->
    (`status`, None)."""

    def get_scales(self, camera, gaussian_model, **kwargs):
        opacities, scales = _mip.filtered_scales_and_opacities(gaussian_model)
        return scales, opacities.squeeze(-1)

    def get_opacities(self, camera, gaussian_model, projections: Tuple, visibility_filter, status: Any, **kwargs):
        return status, None


class HipGSplatMipSplattingRendererV2Module(HipMipSplattingRendererMixin, HipGSplatV1RendererModule):
    pass


@dataclass
class HipGSplatAppearanceEmbeddingMipRenderer(HipGSplatAppearanceEmbeddingRenderer):
    filter_2d_kernel_size: float = 0.1

    def instantiate(self, *args, **kwargs) -> "HipGSplatAppearanceEmbeddingMipRendererModule":
        if self.separate_sh is not True:
            raise ValueError("HipGSplatAppearanceEmbeddingMipRenderer: separate_sh must be True")
        return HipGSplatAppearanceEmbeddingMipRendererModule(self)


class HipGSplatAppearanceEmbeddingMipRendererModule(HipGSplatAppearanceEmbeddingRendererModule):
    """`get_scales` -> (filtered scales, the opacity coefficient as `status`); the appearance model's opacities, offsets included, are
    multiplied by it afterwards, as the reference does."""

    def get_scales(self, camera, gaussian_model, **kwargs):
        return _mip.filtered_scales_and_coef(gaussian_model)

    def get_opacities(self, camera, gaussian_model, projections: Tuple, visibility_filter, status: Any, **kwargs):
        opacity_compensation = status
        opacities, new_status = super().get_opacities(camera, gaussian_model, projections, visibility_filter, None, **kwargs)
        if gaussian_model.config.opacity_compensation:
            opacities = opacities * opacity_compensation
        return opacities, new_status

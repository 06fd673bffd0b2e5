"""HipGSplatAppearanceEmbeddingRenderer — drop-in for the reference's `GSplatAppearanceEmbeddingRenderer`
(internal/renderers/gsplat_appearance_embedding_renderer.py:96-323; configs/appearance.yaml and most of
configs/appearance_embedding_renderer/): per-Gaussian appearance features, one embedding row per appearance id and a small MLP
give each visible Gaussian a colour offset (and, `with_opacity`, an opacity offset) on top of its view-dependent SH colour.

Select with   --model.renderer gspl_amd.renderers.HipGSplatAppearanceEmbeddingRenderer   (INTEGRATION.md).

What runs where, after the warm-up:
  * the MLP is ONE `ops.appearance_mlp` launch over all N rows with the visibility filter as its mask (the reference gathers the
    visible rows with a boolean index, which waits for the row count on the host, repeats the embedding, concatenates and runs
    three Linear layers); `fused_mlp=False`, or a configuration the kernel is not built for, runs the same parameters through
    torch.nn on all rows instead;
  * the base colour is `ops.spherical_harmonics[_decomposed]` with the same mask; the offset, clamp and zero fill are dense torch
    elementwise code.  Nothing is indexed, so no step waits for the device.
During the warm-up the colours are the staged gsplat-v1 plugin's, bit for bit.

The Mip variant is `HipGSplatAppearanceEmbeddingMipRenderer` (hip_gsplat_mip_splatting_renderer.py), which sits on this renderer.
Not built: the distributed, 2DGS and partition-LoD variants of the reference, which subclass this renderer."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Mapping, Tuple

import torch

from .. import ops
from ..appearance import HipAppearanceModel, ModelConfig, OptimizationConfig
from .hip_gsplat_v1_renderer import HipGSplatV1Renderer, HipGSplatV1RendererModule


@dataclass
class HipGSplatAppearanceEmbeddingRenderer(HipGSplatV1Renderer):
    separate_sh: bool = True
    model: ModelConfig = field(default_factory=lambda: ModelConfig())
    optimization: OptimizationConfig = field(default_factory=lambda: OptimizationConfig())
    fused_mlp: bool = True
    """False: the appearance network runs in torch.nn (every configuration does), the rest of the plugin is unchanged."""

    def instantiate(self, *args, **kwargs) -> "HipGSplatAppearanceEmbeddingRendererModule":
        if self.separate_sh is not True:
            raise ValueError("HipGSplatAppearanceEmbeddingRenderer: separate_sh must be True")
        return HipGSplatAppearanceEmbeddingRendererModule(self)


class HipGSplatAppearanceEmbeddingRendererModule(HipGSplatV1RendererModule):
    """rgb = clamp(SH colour + 2 f(appearance features, appearance embedding, view direction) - 1)"""

    opacity_offsets = None
    opacity_offsets_count = None

    def setup(self, stage: str, lightning_module=None, *args: Any, **kwargs: Any) -> Any:
        if lightning_module is None:
            return
        if self.config.model.n_appearances <= 0:
            largest = 0
            group_ids = lightning_module.trainer.datamodule.dataparser_outputs.appearance_group_ids
            if group_ids is not None:
                largest = max([0] + [ids[0] for ids in group_ids.values()])
            self.config.model.n_appearances = largest + 1
        self._setup_model()

    def _setup_model(self, device=None):
        self.model = HipAppearanceModel(self.config.model, fused_mlp=self.config.fused_mlp)
        if device is not None:
            self.model.to(device=device)

    def load_state_dict(self, state_dict: Mapping[str, Any], strict: bool = True):
        """The checkpoint decides the number of appearances: the model is rebuilt with its embedding's row count first."""
        rows = state_dict["model.embedding.weight"]
        self.config.model.n_appearances = rows.shape[0]
        self._setup_model(device=rows.device)
        return super().load_state_dict(state_dict, strict)

    def training_setup(self, module):
        o = self.config.optimization
        shared = dict(lr_final_factor=o.lr_final_factor, max_steps=o.max_steps, eps=o.eps, warm_up=o.warm_up)      # (one final factor for both, as the reference)
        embedding = self._optimizer_and_scheduler(self.model.embedding.parameters(), "embedding", lr_init=o.embedding_lr_init, **shared)
        network = self._optimizer_and_scheduler(self.model.network.parameters(), "embedding_network", lr_init=o.lr_init, **shared)
        if self.config.model.with_opacity:
            module.extra_train_metrics.append(self.opacity_offset_reg)
        return [embedding[0], network[0]], [embedding[1], network[1]]

    @staticmethod
    def _optimizer_and_scheduler(params, name, lr_init, lr_final_factor, max_steps, eps, warm_up):
        optimizer = torch.optim.Adam(params=[{"params": list(params), "name": name}], lr=lr_init, eps=eps)
        scheduler = torch.optim.lr_scheduler.LambdaLR(
            optimizer=optimizer, lr_lambda=lambda iter: lr_final_factor ** min(max(iter - warm_up, 0) / max_steps, 1))
        return optimizer, scheduler

    def opacity_offset_reg(self, outputs, batch, gaussian_model, global_step, pl_module):
        """0.05 x the mean opacity offset of the visible Gaussians: a masked sum over the mask's count, both on the device."""
        if self.opacity_offsets is None:
            return torch.tensor(0., dtype=torch.float, device=pl_module.device)
        loss = self.opacity_offsets.sum() / self.opacity_offsets_count
        pl_module.log("train/opacity_offset_reg", loss, prog_bar=False, on_step=True, on_epoch=False, batch_size=pl_module.batch_size)
        return loss * 0.05

    def sh(self, pc, dirs, mask=None):
        if getattr(pc, "is_pre_activated", False):
            return ops.spherical_harmonics(pc.active_sh_degree, dirs, pc.get_shs(), masks=mask)
        return ops.spherical_harmonics_decomposed(pc.active_sh_degree, dirs, dc=pc.get_shs_dc(), coeffs=pc.get_shs_rest(), masks=mask)

    def get_opacities(self, camera, gaussian_model, projections: Tuple, visibility_filter, status: Any, **kwargs):
        rgbs, opacities, offsets = self._get_rgbs_and_opacities(camera, gaussian_model, projections, visibility_filter, status, **kwargs)
        if self.training:
            self.opacity_offsets = offsets
            self.opacity_offsets_count = None if offsets is None else visibility_filter.sum()
        return opacities, rgbs

    def get_rgbs(self, camera, gaussian_model, projections: Tuple, visibility_filter, status: Any, **kwargs):
        return status

    def _get_rgbs_and_opacities(self, camera, pc, projections: Tuple, visibility_filter, status: Any, **kwargs):
        raw_opacities = pc.get_opacities().squeeze(-1)
        if kwargs.get("warm_up", False):
            return HipGSplatV1RendererModule.get_rgbs(self, camera, pc, projections, visibility_filter, None), raw_opacities, None

        means = pc.get_xyz.detach()
        base_rgbs = self.sh(pc, means - camera.camera_center, visibility_filter) + 0.5
        predicted = self.model(pc.get_appearance_features(), camera.appearance_id, mask=visibility_filter, means=means,
                               camera_center=camera.camera_center)
        visible = visibility_filter.unsqueeze(-1)
        rgb_offsets = predicted[:, :3] * 2 - 1.
        rgbs = torch.where(visible, torch.clamp(base_rgbs + rgb_offsets, min=0., max=1.), 0.)

        opacity_offsets, opacities = None, raw_opacities
        if self.config.model.with_opacity:
            opacity_offsets = torch.where(visibility_filter, predicted[:, 3].float(), 0.)
            opacities = torch.clamp_max(opacity_offsets + raw_opacities, max=1.)
        return rgbs, opacities, opacity_offsets

    def training_forward(self, step: int, module, viewpoint_camera, pc, bg_color: torch.Tensor, scaling_modifier=1.0, **kwargs):
        return self.forward(viewpoint_camera, pc, bg_color, scaling_modifier, warm_up=step < self.config.optimization.warm_up, **kwargs)

"""HipSWAGRenderer — drop-in for the reference's `SWAGRenderer` (internal/renderers/swag_renderer.py, "Splatting in the Wild images
with Appearance-conditioned Gaussians") on the HIP ops: the same constructor fields (`network`, `grid_encoding`, `embedding`,
`optimization`, `temperature`, `eps`), bounding box (the datamodule's point cloud, x 1.1), one Adam + `LambdaLR`, u = 0.5 in
evaluation and one uniform sample per training step, and the vanilla plugin's output dict.

Select with   --model.renderer gspl_amd.renderers.HipSWAGRenderer   (INTEGRATION.md).

What runs where:
  * the view-dependent colours, their +0.5 and clamp are ONE `ops.sh_view_colors` launch whose gradient reaches the means, as
    `eval_gaussian_model_sh` lets it (the reference: a transpose, a repeat, a norm, a division, `eval_sh`, an add and a clamp);
  * the position embedding is `ops.hashgrid_encode` (`tinycudann` has no ROCm build) on the detached, normalised means;
  * F_theta stays `torch.nn` — there is no MLP kernel here — and the opacity variation keeps the reference's order of operations
    (swag_renderer.py:48-53), so both are the reference's bits;
  * the result goes to `ops.GaussianRasterizer` with `colors_precomp`, through `HipVanillaRenderer.render`.
The constants of a call (u = 0.5, the appearance id, the bounding box on the device) are built once, not per frame."""
from __future__ import annotations

from typing import Any

import torch
from torch.distributions.uniform import Uniform

from .. import ops
from ..swag import EmbeddingConfig, GridEncodingConfig, GridEncodingOptimizationConfig, HipSWAGModel, NetworkConfig
from .hip_vanilla_renderer import HipVanillaRenderer
from .renderer import Renderer, model_sh_pair


class HipSWAGRenderer(Renderer):
    def __init__(self, network: NetworkConfig = NetworkConfig(), grid_encoding: GridEncodingConfig = GridEncodingConfig(),
                 embedding: EmbeddingConfig = EmbeddingConfig(), optimization: GridEncodingOptimizationConfig = GridEncodingOptimizationConfig(),
                 temperature: float = 0.1, eps: float = 1e-8) -> None:
        super().__init__()
        self.network_config = network
        self.grid_encoding_config = grid_encoding
        self.embedding_config = embedding
        self.optimization_config = optimization
        self.temperature = temperature
        self.eps = eps
        self._on_device: dict = {}

    def _constant(self, name: str, device):
        """bbox_min / bbox_size / the evaluation u on `device`, copied there once."""
        found = self._on_device.get((name, device))
        if found is None:
            value = torch.tensor(0.5, dtype=torch.float) if name == "u" else getattr(self, name)
            found = self._on_device[(name, device)] = value.to(device)
        return found

    def _get_normalized_xyz(self, gaussian_model):
        xyz = gaussian_model.get_xyz.detach()
        return (xyz - self._constant("bbox_min", xyz.device)) / self._constant("bbox_size", xyz.device)

    def opacity_variation(self, delta_alpha: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
        """swag_renderer.py:48-52, operation for operation; the two terms of u are 1-element tensors."""
        return torch.sigmoid(1 / self.temperature * (
            torch.log(torch.abs(delta_alpha) + self.eps) + torch.log(u + self.eps) - torch.log(1 - u + self.eps)))

    def forward(self, viewpoint_camera, pc, bg_color: torch.Tensor, scaling_modifier=1.0, u=None, **kwargs):
        colors = ops.sh_view_colors(pc.active_sh_degree, pc.get_xyz, viewpoint_camera.camera_center, *model_sh_pair(pc), detach_means=False)
        image_conditioned_colors, image_conditioned_delta_alpha = self.swag_model(
            colors, self._get_normalized_xyz(pc), viewpoint_camera.appearance_id)
        if u is None:          # U is fixed at 0.5 during the evaluation
            u = self._constant("u", bg_color.device)
        variation = self.opacity_variation(image_conditioned_delta_alpha, u)
        final_opacity = torch.clamp_min(pc.get_opacity.squeeze(-1) - variation, 0).unsqueeze(-1)
        return HipVanillaRenderer.render(
            means3D=pc.get_xyz, opacity=final_opacity, scales=pc.get_scaling, rotations=pc.get_rotation, features=None,
            active_sh_degree=pc.active_sh_degree, viewpoint_camera=viewpoint_camera, bg_color=bg_color, scaling_modifier=scaling_modifier,
            colors_precomp=image_conditioned_colors)

    def training_forward(self, step: int, module, viewpoint_camera, pc, bg_color: torch.Tensor, scaling_modifier=1.0, **kwargs):
        return self(viewpoint_camera=viewpoint_camera, pc=pc, bg_color=bg_color, scaling_modifier=scaling_modifier,
                    u=self.uniform_sampler.sample((1,)))

    def setup(self, stage: str, lightning_module=None, *args: Any, xyz=None, **kwargs: Any) -> Any:
        """The scene's size from the datamodule's point cloud (or from `xyz` [P, 3] where there is no trainer), then the model."""
        with torch.no_grad():
            if xyz is None:
                xyz = lightning_module.trainer.datamodule.dataparser_outputs.point_cloud.xyz
            xyz = torch.as_tensor(xyz).detach().cpu()
            self.bbox_min = torch.min(xyz, dim=0).values
            self.bbox_max = torch.max(xyz, dim=0).values
            self.bbox_size = (self.bbox_max - self.bbox_min) * 1.1
            self._on_device.clear()
        self.swag_model = HipSWAGModel(network=self.network_config, grid_encoding=self.grid_encoding_config, embedding=self.embedding_config)

    def training_setup(self, module):
        params = list(self.swag_model.parameters())
        self.uniform_sampler = Uniform(torch.tensor(0, dtype=torch.float, device=params[0].device),
                                       torch.tensor(1, dtype=torch.float, device=params[0].device))
        config = self.optimization_config
        optimizer = torch.optim.Adam(params=[{"params": params, "name": "swag_model"}], lr=config.lr)
        return optimizer, torch.optim.lr_scheduler.LambdaLR(
            optimizer=optimizer, lr_lambda=lambda iter: config.lr_final_factor ** min(iter / config.max_steps, 1))

"""HipVanillaGS4DRenderer — drop-in for the reference's `VanillaGS4DRenderer` (internal/renderers/vanilla_gs4d_renderer.py), the viewer's
`--vanilla_gs4d` route: models trained by 4DGaussians (HexPlane / K-Planes deformation), shown at the camera's `time`.

The same constructor (`model_path`, `load_iteration`, `device`) and the same files: `cfg_args` (the text `Namespace(...)`, read with
`ast`, never evaluated), `point_cloud/iteration_N/deformation.pth` (loaded strictly into `gspl_amd.gs4d.HipDeformNetwork`, whose
names are the reference's) and `deformation_table.pth`.

    GSPL_HIP_GS4D=1 python -m gspl_amd.launch viewer.py <model> --vanilla_gs4d          

What runs where:
  * the HexPlane field — 6 planes x L levels of `F.grid_sample` on channel-major planes, a product chain and a cat in the reference —
    is ONE `ops.hexplane_encode` launch on a channel-last table, at the frame's single time (no [N, 1] tensor of repeated times);
  * the positional embeddings that nothing reads are not computed; the small MLPs stay `torch.nn`;
  * `forward` mirrors the reference's, including that the rasterizer gets `opacity_activation` of the UNDEFORMED opacity
    (vanilla_gs4d_renderer.py:82), and ends in `HipVanillaRenderer.render`."""
from __future__ import annotations

import os

import torch

from ..gs4d import HipDeformNetwork, parse_cfg_args
from .hip_vanilla_renderer import HipVanillaRenderer
from .renderer import Renderer, camera_scalars


class HipVanillaGS4DRenderer(Renderer):
    def __init__(self, model_path: str, load_iteration: int, device) -> None:
        super().__init__()
        self.model_path = model_path
        self.load_iteration = load_iteration
        self.device = device

        self.compute_cov3D_python = False
        self.convert_SHs_python = False

        self.cfg_args = parse_cfg_args(os.path.join(model_path, "cfg_args"))
        checkpoint_dir = os.path.join(model_path, "point_cloud", "iteration_{}".format(load_iteration))
        self.deformation = HipDeformNetwork(self.cfg_args).to(device)
        self.deformation.load_state_dict(torch.load(os.path.join(checkpoint_dir, "deformation.pth"), map_location=device))
        self.deformation.requires_grad_(False)          # a viewer: the packed table is then kept between frames
        self.deformation_table = torch.load(os.path.join(checkpoint_dir, "deformation_table.pth"), map_location=device)

    def forward(self, viewpoint_camera, pc, bg_color: torch.Tensor, scaling_modifier=1.0, **kwargs):
        opacity = pc.opacities
        (time,) = camera_scalars(viewpoint_camera, ("time",))
        means3D_final, scales_final, rotations_final, _, shs_final = self.deformation(
            pc.get_xyz, pc.scales, pc.rotations, opacity, pc.get_features, float(time))
        return HipVanillaRenderer.render(
            means3D=means3D_final,
            opacity=pc.opacity_activation(opacity),          # the reference's: the deformed opacity is computed and not used
            scales=pc.scale_activation(scales_final),
            rotations=pc.rotation_activation(rotations_final),
            features=shs_final,
            active_sh_degree=pc.active_sh_degree,
            viewpoint_camera=viewpoint_camera,
            bg_color=bg_color,
            scaling_modifier=scaling_modifier,
        )

"""HipPeriodicVibrationGaussianRenderer — drop-in for the reference's `PeriodicVibrationGaussianRenderer`
(internal/renderers/periodic_vibration_gaussian_renderer.py; configs/pvg_dynamic.yaml) on the HIP ops: the same configuration
dataclass (`env_map_res`, `anti_aliased`, `time_offset`, `lambda_self_supervision`), `_time_interval` buffer, `training_setup`, random
`time_shift` of `training_forward`, render types and output keys.

Differences that are deliberate:
  * the time-dependent means, the opacity factor and the average velocity are ONE `ops.pvg_motion` launch (the reference: some
    fifteen elementwise launches through four getters), and the camera's `time` travels in a device table instead of being read back;
  * rgb, average velocity, depth and `scale_t` are composited in ONE D = 8 pass over one binning (the reference: up to four complete
    `rasterize_gaussians` calls, each with its own binning and geometry backward); the maps are slices of that image, channels first;
  * the sky is `ops.envlight_blend`: the direction grid, the sky image and the blend never reach memory; `kornia` and `nvdiffrast`
    are not needed;
  * `time_interval` is read back when the buffer changes, not on every shifted step;
  * a request for `average_velocity` or `scale_t` alone still runs the D = 8 pass with the SH colours in it (one form for every wide
    request; the reference would composite that map alone).
As in the reference, render types it does not know select nothing: the maps come back as None, next to the projection's outputs.
The reference's `vanilla_forward` (a modified Inria rasterizer that is pinned nowhere) is not built."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict

import numpy as np
import torch

from .. import ops
from ..envlight import HipEnvLight
from .renderer import Renderer, RendererConfig, RendererOutputInfo, RendererOutputTypes, camera_hw, viewspace_grad_scale, model_sh_pair
from .hip_gsplat_renderer import DEFAULT_BLOCK_SIZE, _project

_WIDE = ("average_velocity", "scale_t")      # the render types that need the D = 8 pass


@dataclass
class HipPeriodicVibrationGaussianRenderer(RendererConfig):
    env_map_res: int = 1024

    anti_aliased: bool = True

    time_offset: float = -0.5

    lambda_self_supervision: float = 0.5

    def instantiate(self, *args, **kwargs) -> "HipPeriodicVibrationGaussianRendererModule":
        return HipPeriodicVibrationGaussianRendererModule(self)


def camera_to_world_rotation(viewpoint_camera) -> torch.Tensor:
    """inv(world_to_camera.T)[:3, :3] as the reference's `get_world_directions` forms it, computed on the device without a read-back
    (`inv_ex`) and kept on the camera object, keyed on the pose tensor's identity and version."""
    w2c = viewpoint_camera.world_to_camera
    cached = getattr(viewpoint_camera, "_gspl_c2w_rotation", None)
    if cached is not None and cached[0] is w2c and cached[1] == w2c._version and not w2c.requires_grad:
        return cached[2]
    rot = torch.linalg.inv_ex(w2c.detach().T.float())[0][:3, :3].contiguous()
    if not w2c.requires_grad:
        try:
            viewpoint_camera._gspl_c2w_rotation = (w2c, w2c._version, rot)
        except Exception:      # a frozen camera type: no cache
            pass
    return rot


class HipPeriodicVibrationGaussianRendererModule(Renderer):
    def __init__(self, config: HipPeriodicVibrationGaussianRenderer) -> None:
        super().__init__()
        self.config = config
        self._interval_cache = None

    @property
    def time_interval(self) -> float:
        cached = self._interval_cache
        if cached is None or cached[0] is not self._time_interval or cached[1] != self._time_interval._version:
            cached = self._interval_cache = (self._time_interval, self._time_interval._version, self._time_interval.item())
        return cached[2]

    @time_interval.setter
    def time_interval(self, v: float):
        self._time_interval.fill_(v)

    def setup(self, stage: str, *args: Any, **kwargs: Any) -> Any:
        self.register_buffer("_time_interval", torch.tensor(0., dtype=torch.float))

        self.env_map = None
        if self.config.env_map_res > 0:
            self.env_map = HipEnvLight(resolution=self.config.env_map_res)
        return super().setup(stage, *args, **kwargs)

    def forward(self, viewpoint_camera, pc, bg_color: torch.Tensor, scaling_modifier=1.0, render_types: list = None,
                time_shift: float = None, **kwargs):
        if render_types is None:
            render_types = ["rgb", "average_velocity"]
        W, H = camera_hw(viewpoint_camera)
        scale_t = pc.get_scale_t()
        means3D, average_velocity, opacities = ops.pvg_motion(
            pc.get_means(), pc.get_velocity(), pc.get_t(), scale_t, pc.get_opacities(), viewpoint_camera.time, pc.config.cycle,
            pc.config.velocity_decay, self.config.time_offset, time_shift)

        xys, depths, radii, conics, comp, num_tiles_hit, _ = _project(
            means3D, pc.get_scaling, pc.get_rotation, viewpoint_camera, scaling_modifier, DEFAULT_BLOCK_SIZE, W, H)
        if self.config.anti_aliased is True:
            opacities = opacities * comp[:, None]
        visible = radii > 0

        need_rgb = any(t in render_types for t in ("rgb", "rgb_without_envmap", "alpha"))
        wide = any(t in render_types for t in _WIDE)
        need_depth = "depth" in render_types
        if not (need_rgb or wide or need_depth):
            # nothing this renderer knows was asked for: as in the reference, every map is None
            return {
                "render": None, "rgb_without_envmap": None, "depth": None, "alpha": None, "average_velocity": None, "scale_t": None,
                "viewspace_points": xys,
                "viewspace_points_grad_scale": viewspace_grad_scale(W, H, xys),
                "visibility_filter": visible,
                "radii": radii,
            }
        columns, background = [], []
        zeros = bg_color.new_zeros((5,))
        if need_rgb or wide:
            # the view directions come from the stored means, detached, as in the reference
            columns.append(ops.sh_view_colors(pc.active_sh_degree, pc.get_xyz, viewpoint_camera.camera_center, *model_sh_pair(pc), visible,
                                              detach_means=True))
            background.append(bg_color)
        if wide:
            columns += [average_velocity, depths[:, None], scale_t.reshape(-1, 1)]
            background.append(zeros)
        elif need_depth:
            columns.append(depths[:, None])
            background.append(zeros[:1])
        colors = columns[0] if len(columns) == 1 else torch.cat(columns, dim=1)
        background = background[0] if len(background) == 1 else torch.cat(background)

        # one binning and one compositing pass for every map (D = 8, or 3 / 4 / 1 when only rgb, alpha and depth are asked for)
        isects = ops.bin_gaussians(xys, depths, radii, H, W, DEFAULT_BLOCK_SIZE, conics=conics, opacities=opacities, lazy=True)
        image, alpha = ops.rasterize_gaussians(xys, depths, radii, conics, num_tiles_hit, colors, opacities, img_height=H, img_width=W,
                                               block_width=DEFAULT_BLOCK_SIZE, background=background, return_alpha=True, isects=isects,
                                               channels_first=True)

        rgb = rgb_without_envmap = alpha_map = depth_map = average_velocity_map = scale_t_map = None
        first = 0
        if need_rgb or wide:
            rgb_without_envmap, first = image[0:3], 3
        if wide:
            average_velocity_map, depth_map, scale_t_map = image[3:6], image[6:7], image[7:8]
        elif need_depth:
            depth_map = image[first:first + 1]
        if need_rgb:
            alpha_map = alpha[None]
            rgb = rgb_without_envmap
            if self.env_map is not None:
                jitter = torch.rand((2, H, W), dtype=torch.float32, device=rgb.device) if self.training else None
                rgb = ops.envlight_blend(rgb_without_envmap, alpha, self.env_map.base, camera_to_world_rotation(viewpoint_camera),
                                         viewpoint_camera.fx, viewpoint_camera.fy, viewpoint_camera.cx, viewpoint_camera.cy, jitter)

        return {
            "render": rgb,
            "rgb_without_envmap": rgb_without_envmap if need_rgb else None,
            "depth": depth_map if need_depth else None,
            "alpha": alpha_map,
            "average_velocity": average_velocity_map if "average_velocity" in render_types else None,
            "scale_t": scale_t_map if "scale_t" in render_types else None,
            "viewspace_points": xys,
            "viewspace_points_grad_scale": viewspace_grad_scale(W, H, xys),
            "visibility_filter": visible,
            "radii": radii,
        }

    def training_forward(self, step: int, module, viewpoint_camera, pc, bg_color: torch.Tensor, render_types: list = None, **kwargs):
        if np.random.random() < self.config.lambda_self_supervision:
            time_shift = 3 * (np.random.random() - 0.5) * self.time_interval
        else:
            time_shift = None

        return self(
            viewpoint_camera=viewpoint_camera,
            pc=pc,
            bg_color=bg_color,
            time_shift=time_shift,
        )

    def training_setup(self, module):
        time_duration = module.gaussian_model.config.time_duration
        frame_num = len(module.trainer.datamodule.dataparser_outputs.train_set)

        self.time_interval = (time_duration[1] - time_duration[0]) / (frame_num - 1)

        return super().training_setup(module)

    def get_available_outputs(self) -> Dict[str, RendererOutputInfo]:
        return {
            "rgb": RendererOutputInfo("render"),
            "rgb_without_envmap": RendererOutputInfo("rgb_without_envmap"),
            "depth": RendererOutputInfo("depth", type=RendererOutputTypes.GRAY),
            "alpha": RendererOutputInfo("alpha", type=RendererOutputTypes.GRAY),
            "average_velocity": RendererOutputInfo("average_velocity", RendererOutputTypes.NORMAL_MAP),
            "scale_t": RendererOutputInfo("scale_t", type=RendererOutputTypes.GRAY),
        }

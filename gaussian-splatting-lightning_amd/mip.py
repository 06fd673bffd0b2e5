"""Mip-Splatting ("Mip-Splatting: Alias-free 3D Gaussian Splatting") as a plugin of the reference's training loop: the model that
carries a per-Gaussian 3D filter and the functions that compute and apply it (internal/models/mip_splatting.py;
configs/mip_splatting_gsplat_v2*.yaml).  The same YAML selects it with the class paths changed:

    --model.gaussian gspl_amd.mip.HipMipSplatting
    --model.renderer gspl_amd.renderers.HipGSplatMipSplattingRendererV2

The 2D half (the `filter_2d_kernel_size` dilation and the `anti_aliased` compensation) is the projection kernels'; this is the 3D half.
The reference computes the filter with a Python loop over every training camera, about twenty elementwise launches and two
boolean-index assignments (host waits) per camera, and applies it every step with a dozen elementwise launches on top of the ten of
the model's activations.  Here:

compute_3d_filter(cameras, gaussian_model), apply_3d_filter(...), apply_3d_filter_on_scales(...)
    stand-ins with the signatures of the reference's `MipSplattingUtils` (also as `HipMipSplattingUtils`), on `ops.mip_filter_3d` (two
    launches for all cameras, nothing read by the host) and `ops.mip_apply_3d_filter` (one launch, one more in the backward).
filtered_scales_and_opacities(model), filtered_scales_and_coef(model)
    ONE `ops.mip_apply_3d_filter` call for a model that carries a filter, the reference's `MipSplattingModel` included: with the
    model's RAW scales and opacities, the exp and the sigmoid inside the kernel, when its `scale_activation` / `opacity_activation` are
    the reference vanilla model's own; through its getters otherwise.  The renderer plugins call these.
HipMipSplatting / HipMipSplattingModel
    the reference's `MipSplatting` / `MipSplattingModel` (their fields, property name `filter_3d`, state-dict keys: a checkpoint of
    either loads strictly into the other) with `training_setup` building the camera table once on the model's device,
    `compute_3d_filter` one op call on that table and `get_3d_filtered_scales_and_opacities` the fused call.  Their base is the
    reference's own model; stand-alone there is no such base and `instantiate` says so.

Tensors on the CPU take the ops' plain-torch restatement, the reference's operations bit for bit.  Differences from the reference
(ops/mip.py has the detail): a scene in which no camera sees any Gaussian keeps 100000 as every distance instead of raising, and on
the GPU the opacity coefficient stays finite for scales below about 1e-7.

Not built: the old `MipSplattingGSplatRenderer` (filter kept in the renderer), the distributed appearance-Mip renderer, partition-LoD
tables of Mip models (`LoDTable` refuses them), half precision."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import ops
from .renderers.renderer import _defined_by_reference_vanilla_model

BASE_NAME = "internal.models.mip_splatting"
try:  # pragma: no cover - only inside the reference repo (needs lightning)
    from internal.models.mip_splatting import MipSplatting, MipSplattingModel, MipSplattingModelMixin  # type: ignore
    INSIDE_REFERENCE = True
except Exception:
    INSIDE_REFERENCE = False
    MipSplattingModel = MipSplattingModelMixin = None

    @dataclass
    class MipSplatting:
        """The two fields Mip-Splatting adds to the reference's `VanillaGaussian` (the others come with that base, inside the
        reference)."""
        filter_3d_update_interval: int = 100

        opacity_compensation: bool = True


# ---- the reference's three functions ----------------------------------------------------------------------------------------------------
@torch.no_grad()
def compute_3d_filter(cameras, gaussian_model, camera_table: Optional[torch.Tensor] = None) -> torch.nn.Parameter:
    """`MipSplattingUtils.compute_3d_filter` -> Parameter [N, 1], requires_grad=False.  `cameras`: an iterable of cameras (a tqdm
    wrapper is fine); `camera_table`: the `ops.mip_camera_table` of them when the caller keeps one (then `cameras` is not read)."""
    xyz = gaussian_model.get_xyz
    if camera_table is None:
        camera_table = ops.mip_camera_table(cameras, xyz.device)
    return torch.nn.Parameter(ops.mip_filter_3d(xyz, camera_table.to(xyz.device)), requires_grad=False)


def apply_3d_filter_on_scales(filter_3d: torch.Tensor, scales: torch.Tensor, compute_opacity_compensation: bool = True
                              ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """-> (filtered scales [N, 3], the opacity coefficient [N] or None)"""
    return ops.mip_apply_3d_filter(scales, filter_3d, None, opacity_compensation=compute_opacity_compensation)


def apply_3d_filter(filter_3d: torch.Tensor, opacities: torch.Tensor, scales: torch.Tensor, opacity_compensation: bool = True
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (opacities [N, 1], filtered scales [N, 3]), the reference's order"""
    new_scales, new_opacities = ops.mip_apply_3d_filter(scales, filter_3d, opacities, opacity_compensation=opacity_compensation)
    return new_opacities, new_scales


class HipMipSplattingUtils:
    compute_3d_filter = staticmethod(compute_3d_filter)
    apply_3d_filter_on_scales = staticmethod(apply_3d_filter_on_scales)
    apply_3d_filter = staticmethod(apply_3d_filter)


# ---- a model's filtered scales and opacities in one call --------------------------------------------------------------------------------
def _stored_or_activated(model, name: str, activation: str, getter: str):
    """(tensor, raw): the STORED parameter, to be activated inside the kernel, when `activation` is the reference vanilla model's own
    method and `getter` the reference base class's (so that the kernel's exp / sigmoid IS what the getter would compute); what the
    getter returns otherwise (a pre-activated model, another activation, a model of another family)."""
    if not getattr(model, "is_pre_activated", False) and _defined_by_reference_vanilla_model(getattr(model, activation, None), activation):
        get = getattr(type(model), getter, None)
        module = getattr(get, "__module__", "") or ""
        if module == "internal.models.gaussian" or module.endswith(".internal.models.gaussian"):
            try:
                return model.get_property(name), True
            except (KeyError, AttributeError):
                pass
    return getattr(model, getter)(), False


def _filter_of(model) -> torch.Tensor:
    if not hasattr(model, "get_3d_filter"):
        raise TypeError(f"{type(model).__name__} carries no 3D filter (`get_3d_filter`): the Mip-Splatting renderers need the reference's "
                        "MipSplatting model or gspl_amd.mip.HipMipSplatting")
    return model.get_3d_filter()


def filtered_scales_and_opacities(model) -> Tuple[torch.Tensor, torch.Tensor]:
    """`MipSplattingModelMixin.get_3d_filtered_scales_and_opacities` in one op call -> (opacities [N, 1], scales [N, 3])."""
    scales, raw_scales = _stored_or_activated(model, "scales", "scale_activation", "get_scales")
    opacities, raw_opacities = _stored_or_activated(model, "opacities", "opacity_activation", "get_opacities")
    new_scales, new_opacities = ops.mip_apply_3d_filter(scales, _filter_of(model), opacities, raw_scales=raw_scales, raw_opacities=raw_opacities,
                                                        opacity_compensation=model.config.opacity_compensation)
    return new_opacities, new_scales


def filtered_scales_and_coef(model) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """`apply_3d_filter_on_scales` on the model's filter and scales in one op call -> (scales [N, 3], coef [N] or None)."""
    scales, raw_scales = _stored_or_activated(model, "scales", "scale_activation", "get_scales")
    return ops.mip_apply_3d_filter(scales, _filter_of(model), None, raw_scales=raw_scales, opacity_compensation=model.config.opacity_compensation)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
@dataclass
class HipMipSplatting(MipSplatting):
    def instantiate(self, *args, **kwargs) -> "HipMipSplattingModel":
        if not INSIDE_REFERENCE:
            raise RuntimeError(f"gspl_amd.mip.HipMipSplatting builds on {BASE_NAME} (MipSplattingModel: the vanilla model's properties, "
                               "optimizers and checkpoint format plus the `filter_3d` property), which is not importable here: run it "
                               "inside the reference repository.  compute_3d_filter, apply_3d_filter, apply_3d_filter_on_scales, "
                               "filtered_scales_and_opacities and filtered_scales_and_coef of this module work without it.")
        return HipMipSplattingModel(self)


if INSIDE_REFERENCE:  # pragma: no cover - only inside the reference repo
    class HipMipSplattingModel(MipSplattingModel):
        config: HipMipSplatting

        def training_setup(self, module):
            device = self.get_means().device
            # the table takes the place of the reference's `_train_camera_set` (every camera moved to the device and kept there)
            self._camera_table = ops.mip_camera_table(module.trainer.datamodule.dataparser_outputs.train_set.cameras, device)
            self.compute_3d_filter()
            return super(MipSplattingModelMixin, self).training_setup(module)

        def compute_3d_filter(self):
            self.gaussians[self._filter_3d_name] = compute_3d_filter(None, self, camera_table=self._camera_table)

        def get_3d_filtered_scales_and_opacities(self):
            return filtered_scales_and_opacities(self)
else:
    HipMipSplattingModel = None

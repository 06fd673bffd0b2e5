"""3DGS-MCMC (Kheradmand et al., "3D Gaussian Splatting as Markov Chain Monte Carlo") as plugins of the reference's training loop.

The reference's route (configs/mcmc.yaml, configs/gsplat-mcmc.yaml) cannot be loaded on ROCm: its controller module begins with
`from gsplat.relocation import compute_relocation` (internal/density_controllers/mcmc_density_controller.py:13), a CUDA kernel
with no ROCm build, which the `gsplat` stand-in of `gspl_amd.compat` deliberately does not provide.  These classes take its place:

    --model.density gspl_amd.mcmc.HipMCMCDensityController --model.density.cap_max 1000000
    --model.metric gspl_amd.mcmc.HipMCMCMetrics

HipMCMCDensityController   the reference's `MCMCDensityController` restated (same fields, defaults and behaviour, :20-236), with
    `compute_relocation` on the HIP op and `_add_xyz_noise` as ONE launch (`ops.perturb_means_`) instead of compute_cov_3d +
    randn_like + sigmoid + bmm.  The bookkeeping — nonzero, multinomial, bincount, the indexed writes and the optimizer surgery —
    is the reference's torch code in the reference's order, so that the same torch seed samples the same indices.
HipMCMCMetrics             the reference's `MCMCMetrics` with `reg_loss` on `ops.mcmc_regularization` (one reduction launch and one
    elementwise backward instead of two activations, two means and their backward).

Inside the reference tree the bases are the reference's own classes; stand-alone (tests, this package's loops) they are
interface-identical stubs, as in renderers/renderer.py."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Tuple

import torch

from . import optim_utils
from .ops import mcmc as _ops
from .renderers.renderer import model_raw_parameters

try:  # pragma: no cover - only inside the reference repo (needs lightning)
    from internal.density_controllers.density_controller import DensityController, DensityControllerImpl  # type: ignore
    INSIDE_REFERENCE = True
except Exception:
    INSIDE_REFERENCE = False

    class DensityControllerImpl(torch.nn.Module):
        """Same surface as the reference's `DensityControllerImpl` (internal/density_controllers/density_controller.py:8-29)."""

        def __init__(self, config, *args, **kwargs) -> None:
            super().__init__()
            self.config = config

        def before_backward(self, outputs, batch, gaussian_model, optimizers, global_step: int, pl_module) -> None:
            pass

        def after_backward(self, outputs, batch, gaussian_model, optimizers, global_step: int, pl_module) -> None:
            pass

        def setup(self, stage: str, pl_module) -> None:
            pass

        def on_load_checkpoint(self, module, checkpoint):
            pass

        def after_density_changed(self, gaussian_model, optimizers, pl_module) -> None:
            pass

    class DensityController:
        def instantiate(self, *args, **kwargs) -> DensityControllerImpl:
            raise NotImplementedError()


def _inverse_sigmoid(x):
    return torch.log(x / (1 - x))        # internal/utils/general_utils.py


@dataclass
class HipMCMCDensityController(DensityController):
    cap_max: int
    """the maximum number of Gaussians"""

    noise_lr: float = 5e5

    densify_from_iter: int = 500

    densify_until_iter: int = 25_000

    densification_interval: int = 100

    min_opacity: float = 0.005

    N_max: int = 51

    def instantiate(self, *args, **kwargs) -> DensityControllerImpl:
        assert self.cap_max > 0, "cap_max must > 0"
        return HipMCMCDensityControllerImpl(self)


class HipMCMCDensityControllerImpl(DensityControllerImpl):
    config: HipMCMCDensityController

    def setup(self, stage: str, pl_module) -> None:
        super().setup(stage, pl_module)
        N_max = self.config.N_max
        binoms = torch.zeros((N_max, N_max), dtype=torch.float, device=pl_module.device)
        for n in range(N_max):
            for k in range(n + 1):
                binoms[n, k] = math.comb(n, k)
        self.register_buffer("binoms", binoms, persistent=False)
        if stage == "fit":
            self._opacities_and_scales_initialization(pl_module.gaussian_model)
        pl_module.on_train_batch_end_hooks.append(self._add_xyz_noise)

    @staticmethod
    def _opacities_and_scales_initialization(gaussian_model) -> None:
        with torch.no_grad():
            scales, opacities = gaussian_model.get_property("scales"), gaussian_model.get_property("opacities")
            scales.copy_(scales + math.log(0.1))
            opacities.copy_(_inverse_sigmoid(torch.ones_like(opacities) * 0.5))

    def after_backward(self, outputs: dict, batch, gaussian_model, optimizers, global_step: int, pl_module) -> None:
        if global_step >= self.config.densify_until_iter:
            return
        if global_step <= self.config.densify_from_iter:
            return
        if global_step % self.config.densification_interval != 0:
            return
        with torch.no_grad():
            dead_mask = (gaussian_model.get_opacities() <= self.config.min_opacity).squeeze(-1)
            self.relocate_gs(gaussian_model, optimizers, dead_mask)
            self.add_new_gs(gaussian_model, optimizers)

    @staticmethod
    def _means_lr(pl_module) -> float:
        xyz_lr = -1
        for opt in pl_module.gaussian_optimizers:
            for param_group in opt.param_groups:
                if param_group["name"] == "means":
                    xyz_lr = param_group["lr"]
            if xyz_lr >= 0:
                break
        assert xyz_lr >= 0
        return xyz_lr

    def _add_xyz_noise(self, outputs: dict, batch, gaussian_model, global_step: int, pl_module) -> None:
        # The reference's guard, kept as it is: `is_final_step` is a METHOD of the LightningModule (gaussian_splatting.py:283), so
        # `pl_module.is_final_step is True` never holds and the noise is added after every step, the last one included.
        if pl_module.is_final_step is True:
            return
        coeff = self.config.noise_lr * self._means_lr(pl_module)
        means = gaussian_model.get_property("means")
        raw = model_raw_parameters(gaussian_model)
        with torch.no_grad():
            if raw is not None:
                scales, rotations, opacities = raw
                _ops.perturb_means_(means, scales, rotations, opacities, raw=True, noise_scale=coeff)
            else:
                _ops.perturb_means_(means, gaussian_model.get_scales().contiguous(), gaussian_model.get_rotations().contiguous(),
                                    gaussian_model.get_opacities().contiguous(), raw=False, noise_scale=coeff)

    def compute_relocation(self, opacity_old, scale_old, N) -> Tuple[torch.Tensor, torch.Tensor]:
        return _ops.compute_relocation(opacity_old.contiguous(), scale_old.contiguous(), N.contiguous(), self.binoms)

    def _get_new_params(self, gaussian_model, idxs, ratio) -> Dict[str, torch.Tensor]:
        new_opacity, new_scaling = self.compute_relocation(
            opacity_old=gaussian_model.get_opacities()[idxs, 0],
            scale_old=gaussian_model.get_scales()[idxs],
            N=ratio[idxs, 0] + 1,
        )
        new_opacity = torch.clamp(new_opacity.unsqueeze(-1), max=1.0 - torch.finfo(torch.float32).eps, min=0.005)
        new_opacity = gaussian_model.opacity_inverse_activation(new_opacity)
        new_scaling = gaussian_model.scale_inverse_activation(new_scaling.reshape(-1, 3))
        new_params = {"opacities": new_opacity, "scales": new_scaling}
        for attr_name, value in gaussian_model.properties.items():
            if attr_name not in new_params:
                new_params[attr_name] = value[idxs]
        return new_params

    @staticmethod
    def _sample_alives(probs, num, alive_indices=None):
        probs = probs / (probs.sum() + torch.finfo(torch.float32).eps)
        sampled_idxs = torch.multinomial(probs, num, replacement=True)
        if alive_indices is not None:
            sampled_idxs = alive_indices[sampled_idxs]
        ratio = torch.bincount(sampled_idxs).unsqueeze(-1)
        return sampled_idxs, ratio

    @staticmethod
    def replace_tensors_to_optimizers(gaussian_model, optimizers, inds=None):
        gaussian_model.properties = optim_utils.replace_tensors_to_properties(gaussian_model.properties, optimizers, selector=inds)

    def relocate_gs(self, gaussian_model, optimizers, dead_mask):
        if dead_mask.sum() == 0:
            return
        alive_mask = ~dead_mask
        dead_indices = dead_mask.nonzero(as_tuple=True)[0]
        alive_indices = alive_mask.nonzero(as_tuple=True)[0]
        if alive_indices.shape[0] <= 0:
            return
        probs = gaussian_model.get_opacities()[alive_indices, 0]
        reinit_idx, ratio = self._sample_alives(alive_indices=alive_indices, probs=probs, num=dead_indices.shape[0])
        new_params = self._get_new_params(gaussian_model, reinit_idx, ratio=ratio)
        for attr_name in new_params:
            gaussian_model.get_property(attr_name)[dead_indices] = new_params[attr_name]
        opacities, scales = gaussian_model.get_property("opacities"), gaussian_model.get_property("scales")
        opacities[reinit_idx] = opacities[dead_indices]
        scales[reinit_idx] = scales[dead_indices]
        self.replace_tensors_to_optimizers(gaussian_model, optimizers=optimizers, inds=reinit_idx)

    def add_new_gs(self, gaussian_model, optimizers):
        cap_max = self.config.cap_max
        current_num_points = gaussian_model.n_gaussians
        target_num = min(cap_max, int(1.05 * current_num_points))
        num_gs = max(0, target_num - current_num_points)
        if num_gs <= 0:
            return 0
        probs = gaussian_model.get_opacities().squeeze(-1)
        add_idx, ratio = self._sample_alives(probs=probs, num=num_gs)
        new_params = self._get_new_params(gaussian_model, add_idx, ratio=ratio)
        gaussian_model.get_property("opacities")[add_idx] = new_params["opacities"]
        gaussian_model.get_property("scales")[add_idx] = new_params["scales"]
        gaussian_model.properties = optim_utils.cat_tensors_to_properties(new_params, gaussian_model, optimizers)
        self.replace_tensors_to_optimizers(gaussian_model, optimizers=optimizers, inds=add_idx)
        return num_gs


# ---- the regulariser ----------------------------------------------------------------------------------------------------------------
try:  # pragma: no cover - only inside the reference repo (internal/metrics imports lightning-free modules, but needs the tree)
    from internal.metrics.mcmc_metrics import MCMCMetrics as _MCMCMetrics, MCMCMetricsImpl as _MCMCMetricsImpl  # type: ignore
except Exception:
    _MCMCMetrics = _MCMCMetricsImpl = None


def hip_reg_loss(metric, gaussian_model, basic_metrics):
    """`MCMCMetricsModuleMixin.reg_loss` (internal/metrics/mcmc_metrics.py) on `ops.mcmc_regularization`: the same two terms, the same
    logged entries.  On the reference's vanilla model the raw parameters go in and the activations happen inside the kernels."""
    raw = model_raw_parameters(gaussian_model)
    if raw is not None:
        scales, _, opacities = raw
    else:
        scales, opacities = gaussian_model.get_scaling, gaussian_model.get_opacity
    scale_w = metric.scale_reg_weight if metric.scale_reg_weight > 0 else 0.
    opacity_reg_loss, scale_reg_loss = _ops.mcmc_regularization(opacities, scales, metric.opacity_reg_weight, scale_w, raw=raw is not None)
    if not metric.scale_reg_weight > 0:
        scale_reg_loss = 0.
    basic_metrics[0]["loss"] = basic_metrics[0]["loss"] + opacity_reg_loss + scale_reg_loss
    basic_metrics[0]["o_reg"] = opacity_reg_loss
    basic_metrics[0]["s_reg"] = scale_reg_loss
    basic_metrics[1]["o_reg"] = False
    basic_metrics[1]["s_reg"] = False
    return basic_metrics


if _MCMCMetrics is not None:
    class HipMCMCMetricsImpl(_MCMCMetricsImpl):
        def reg_loss(self, gaussian_model, basic_metrics):
            return hip_reg_loss(self, gaussian_model, basic_metrics)

    @dataclass
    class HipMCMCMetrics(_MCMCMetrics):
        def instantiate(self, *args, **kwargs):
            return HipMCMCMetricsImpl(self)
else:
    @dataclass
    class HipMCMCMetrics:
        """Stand-alone placeholder: the metric subclasses the reference's `MCMCMetrics` and needs the reference tree."""
        mcmc_reg_until_iter: int = -1
        opacity_reg: float = 0.01
        scale_reg: float = 0.01
        reg_weight_decay: float = 1.

        def instantiate(self, *args, **kwargs):
            raise RuntimeError("gspl_amd.mcmc.HipMCMCMetrics subclasses internal.metrics.mcmc_metrics.MCMCMetrics: run it inside the "
                               "reference repository")

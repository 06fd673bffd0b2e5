"""Taming-3DGS ("Taming 3DGS: High-Quality Radiance Fields with Limited Resources") density control as a plugin of the reference's
training loop: the budget curve, the per-Gaussian importance score summed over sampled training views, and score-driven cloning,
splitting and pruning.

The reference's controller (internal/density_controllers/taming_3dgs_density_controller.py) cannot be loaded here: its module imports
`torchvision.transforms` and PIL for a 3x3 edge filter on the CPU, and its scoring calls `Taming3DGSUtils.normalize` nine times per
view — each an in-place NaN write, a boolean gather (a host wait), a sort-based `torch.median` and a masked scatter.  These classes
take its place; the same YAML selects them with the class path changed:

    --model.density gspl_amd.taming.HipTaming3DGSDensityController --model.density.budget 15
    --model.renderer gspl_amd.renderers.HipGSplatV1Renderer

HipTaming3DGSDensityController   the reference's `Taming3DGSDensityController` (same fields, defaults and `ScoreCoefficients`, :19-87).
HipTaming3DGSDensityControllerImpl   `Taming3DGSDensityControllerModule` restated (:90-362): the edge maps by `ops.find_edges` and kept
    on the device (`edges_on_cpu=True` parks them on the host as the reference does), the score by `compute_gaussian_score` below;
    `_densify_and_prune_with_scores`, `_densify_and_clone`, `_densify_and_split`, `_opacity_culling` and `update_states` in the
    reference's order, every random draw in its order and on its device (the `torch.multinomial` of `_opacity_culling` on the CPU), so
    that the same torch seed selects the same rows.  Its base is the reference's own `VanillaDensityControllerImpl`:
    `_split_properties`, `_densification_postfix`, `_prune_points`, `_add_densification_stats` and the schedule are the reference's
    code.  Stand-alone there is no such base and `instantiate` says so.

Free functions, usable anywhere: `count_array` (:376-395), `edge_maps` (:132-140), `loss_map` (:410-419), `photometric_loss` (:398-407)
and `compute_gaussian_score` (:468-555).

Not built: the feed-forward variant (taming_3dgs_density_ff_controller.py), GNS (needs `rasterize_to_vis_aware_weights`, another
kernel), the Inria-API `vanilla_rasterize_to_weights` path (never called by the reference's own `compute_gaussian_score`), masks in the
edge maps (a TODO in the reference too) and half precision."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Literal, Optional, Tuple

import torch

from . import ops
from .ops import taming as _ops

BASE_NAME = "internal.density_controllers.vanilla_density_controller.VanillaDensityControllerImpl"
try:  # pragma: no cover - only inside the reference repo (needs lightning)
    from internal.density_controllers.density_controller import DensityController  # type: ignore
    from internal.density_controllers.vanilla_density_controller import VanillaDensityControllerImpl  # type: ignore
    INSIDE_REFERENCE = True
except Exception:
    INSIDE_REFERENCE = False
    VanillaDensityControllerImpl = None

    class DensityController:
        def instantiate(self, *args, **kwargs):
            raise NotImplementedError()


@dataclass
class ScoreCoefficients:
    view_importance: float = 50
    edge_importance: float = 50
    mse_importance: float = 50
    grad_importance: float = 25
    dist_importance: float = 50
    opac_importance: float = 100
    dept_importance: float = 5
    loss_importance: float = 10
    radii_importance: float = 10
    scale_importance: float = 25
    count_importance: float = 0.1
    blend_importance: float = 50


@dataclass
class HipTaming3DGSDensityController(DensityController):
    percent_dense: float = 0.01

    densification_interval: int = 500

    opacity_reset_interval: int = 3000

    densify_from_iter: int = 500

    densify_until_iter: int = 15_000

    densify_grad_threshold: float = 0.0002

    cull_opacity_threshold: float = 0.005
    """threshold of opacity for culling gaussians."""

    opacity_correction: bool = False

    cull_by_max_opacity: bool = False

    cull_big_scale: bool = True

    camera_extent_factor: float = 1.

    scene_extent_override: float = -1.

    absgrad: bool = False

    acc_vis: bool = False

    # Taming3DGS hyperparameters

    n_sample_cameras: int = 10

    mode: Literal["multiplier", "final_count"] = "multiplier"

    start_count: int = -1

    budget: float = 20

    cull_opacity_until: int = 27

    score_coeffs: ScoreCoefficients = field(default_factory=ScoreCoefficients)

    # Altitude

    up_direction: Tuple[float, float, float] = None

    min_alt: float = None

    # this package's (not a field of the reference)

    edges_on_cpu: bool = False
    """park the edge maps on the host between densification events, as the reference does (one copy per sampled view and event)"""

    def instantiate(self, *args, **kwargs) -> "HipTaming3DGSDensityControllerImpl":
        if not INSIDE_REFERENCE:
            raise RuntimeError(f"gspl_amd.taming.HipTaming3DGSDensityController builds on {BASE_NAME} (its _split_properties, "
                               "_densification_postfix, _prune_points, _add_densification_stats and schedule), which is not importable "
                               "here: run it inside the reference repository.  count_array, edge_maps, loss_map and "
                               "compute_gaussian_score of this module work without it.")
        return HipTaming3DGSDensityControllerImpl(self)


# ---- free functions -------------------------------------------------------------------------------------------------------------------
def count_array(start_count, multiplier, densify_until_iter, densify_from_iter, densification_interval, mode) -> List[int]:
    """`Taming3DGSUtils.get_count_array` (:376-395): the Gaussian budget of every densification event, Eq. (2) of the paper.  Pure
    Python, with the reference's int() truncations."""
    if mode == "multiplier":
        budget = int(start_count * float(multiplier))
    elif mode == "final_count":
        budget = multiplier
    else:
        raise ValueError(f"count_array: mode must be 'multiplier' or 'final_count', got {mode!r}")

    num_steps = (densify_until_iter + densification_interval - 1) // densification_interval - densify_from_iter // densification_interval

    increasable = max(budget - start_count, 0)
    slope_lower_bound = increasable / num_steps

    k = 2 * slope_lower_bound
    a = (increasable - k * num_steps) / (num_steps * num_steps)
    b = k
    c = start_count

    return [int(1 * a * (x**2) + (b * x) + c) for x in range(num_steps)]


def edge_maps(train_set, device=None, on_cpu: bool = False) -> List[torch.Tensor]:
    """One normalised edge map [H, W] per training image (`on_train_start`, :132-140): `item[1][1]` is the image, uint8 or float in
    [0, 1].  `device`: where `ops.find_edges` runs (default: where the image is; the GPU takes the HIP kernels).  The maps stay there
    unless `on_cpu`."""
    maps = []
    for item in train_set:
        image = item[1][1]
        if device is not None:
            image = image.to(device=device)
        if image.dtype != torch.uint8:
            image = image.to(torch.float32)
        edges = ops.find_edges(image.contiguous())
        maps.append(edges.cpu() if on_cpu else edges)
    return maps


def photometric_loss(a, b, lambda_dssim: float, mask=None) -> torch.Tensor:
    """`compute_photometric_loss` (:398-407) with this package's `fused_ssim`; a 0-dim tensor on the images' device."""
    if mask is not None:
        mask = mask.to(device=a.device, dtype=torch.uint8)
        a = a * mask
        b = b * mask
    l1 = torch.abs(a - b).mean()
    ssim = ops.fused_ssim(a.unsqueeze(0), b.unsqueeze(0), train=False)
    return (1. - lambda_dssim) * l1 + lambda_dssim * (1. - ssim)


def loss_map(reconstructed_image, original_image, config, edges_loss_norm) -> torch.Tensor:
    """`get_loss_map` (:410-419): the channel mean of |render - gt|, min-max normalised, times `mse_importance`, plus
    `edge_importance` x the edge map.  Torch ops, three small reductions, nothing read by the host."""
    l1_loss = torch.mean(torch.abs(reconstructed_image - original_image), 0).detach()
    lo, hi = torch.aminmax(l1_loss)
    l1_loss_norm = (l1_loss - lo) / (hi - lo)
    return (config.mse_importance * l1_loss_norm) + (config.edge_importance * edges_loss_norm)


# the rows of a view in the reference's order of addition (:536-549): five per Gaussian, then four per pixel
PER_GAUSSIAN = ("grad_importance", "opac_importance", "dept_importance", "radii_importance", "scale_importance")
PER_PIXEL = ("dist_importance", "loss_importance", "count_importance", "blend_importance")


def score_rows(all_grads, all_opacity, all_depths, all_radii, all_scales, dist_accum, loss_accum, reverse_counts, blending_weights):
    return [all_grads, all_opacity, all_depths, all_radii, all_scales, dist_accum, loss_accum, reverse_counts, blending_weights]


def score_coefficients(score_coeffs) -> List[float]:
    return [float(getattr(score_coeffs, name)) for name in PER_GAUSSIAN + PER_PIXEL]


def rasterize_to_weights(opacities, projections, isects, pixel_weights, viewpoint_camera):
    """`Taming3DGSUtils.rasterize_to_weights` (:421-441) on `ops.rasterize_to_weights`."""
    from .renderers.hip_gsplat_v1_renderer import GSplatV1
    img_width, img_height = GSplatV1.preprocess_camera(viewpoint_camera)[-1]
    radii, means2d, depths, conics, _ = projections
    _, _, flatten_ids, isect_offsets = isects
    accum_weights, reverse_counts, blend_weights, dist_accum = ops.rasterize_to_weights(
        means2d=means2d, conics=conics, opacities=opacities.unsqueeze(0), image_width=img_width, image_height=img_height, tile_size=16,
        isect_offsets=isect_offsets, flatten_ids=flatten_ids, pixel_weights=pixel_weights.unsqueeze(0))
    return depths[0], radii[0], accum_weights[0], reverse_counts[0], blend_weights[0], dist_accum[0]


_NEEDED_OUTPUTS = ("render", "opacities", "visibility_filter", "projections", "isects")


@torch.no_grad()
def compute_gaussian_score(gaussian_model, renderer, global_steps: int, all_grads: torch.Tensor, sample_cameras: List,
                           edge_losses: List[torch.Tensor], bg_color: torch.Tensor, score_coeffs, lambda_dssim: float,
                           medians_op=None, accumulate_op=None, weights_op=None) -> torch.Tensor:
    """`Taming3DGSUtils.compute_gaussian_score` (:468-555), the reference's signature and loop -> importance [N] float32.

    Per view: one `training_forward`, the photometric loss, the loss map, `rasterize_to_weights`, ONE `ops.positive_medians` over the
    nine rows and ONE `ops.taming_score_accumulate_`; `all_depths` is masked by visibility before its median, as in the reference
    (out of place: the renderer's depths are left alone).  After the renderer returns nothing waits for the device: no `.item()`,
    `.cpu()` or boolean gather; the view's weight `view_importance * photometric_loss` stays a device scalar.
    medians_op / accumulate_op / weights_op: stand-ins for the three ops (tests)."""
    medians_op = medians_op or ops.positive_medians
    accumulate_op = accumulate_op or ops.taming_score_accumulate_
    weights_op = weights_op or rasterize_to_weights
    num_points = gaussian_model.n_gaussians if hasattr(gaussian_model, "n_gaussians") else gaussian_model.get_means().shape[0]
    gaussian_importance = torch.zeros((num_points,), device=bg_color.device, dtype=torch.float32)

    # Is MipSplatting?
    if hasattr(gaussian_model, "get_3d_filtered_scales_and_opacities"):
        _, all_scales = gaussian_model.get_3d_filtered_scales_and_opacities()
    else:
        all_scales = gaussian_model.get_scales()
    all_scales = torch.prod(all_scales.detach().to(torch.float32), dim=1)
    all_grads = all_grads.detach().to(torch.float32).reshape(-1).contiguous()
    coeffs = score_coefficients(score_coeffs)

    for camera_idx in range(len(sample_cameras)):
        camera, image_info, _ = sample_cameras[camera_idx]
        _, gt_image, masked_pixels = image_info

        gt_image = gt_image.to(device=bg_color.device)
        if gt_image.dtype == torch.uint8:
            gt_image = gt_image.to(dtype=bg_color.dtype) / 255.

        # appearance model has warm up, so invoke `training_forward` is required
        outputs = renderer.training_forward(global_steps, None, camera, gaussian_model, bg_color, render_types=["rgb"])
        missing = [k for k in _NEEDED_OUTPUTS if outputs.get(k) is None]
        if missing:
            raise RuntimeError(f"compute_gaussian_score: the renderer's output lacks {missing}; the Taming score needs a renderer whose "
                               "output carries `opacities`, `projections` and `isects` (gspl_amd.renderers.HipGSplatV1Renderer does)")
        render_image = outputs["render"].detach()
        all_opacity = outputs["opacities"].detach()
        visibility_filter = outputs["visibility_filter"]

        w = score_coeffs.view_importance * photometric_loss(render_image, gt_image, lambda_dssim, masked_pixels)
        pixel_weights = loss_map(render_image, gt_image, score_coeffs, edge_losses[camera_idx].to(device=bg_color.device))  # [H, W]

        all_depths, all_radii, loss_accum, reverse_counts, blending_weights, dist_accum = weights_op(
            opacities=all_opacity, projections=outputs["projections"], isects=outputs["isects"], pixel_weights=pixel_weights,
            viewpoint_camera=camera)

        # In gsplat, only the visible Gaussians have valid depth values
        all_depths = all_depths.detach() * visibility_filter

        rows = score_rows(all_grads, all_opacity.contiguous(), all_depths, all_radii.contiguous(), all_scales, dist_accum, loss_accum,
                          reverse_counts, blending_weights)
        counts, medians = medians_op(rows)
        accumulate_op(gaussian_importance, rows, coeffs, counts, medians, w.to(torch.float32), visibility_filter, n_first=len(PER_GAUSSIAN))

    return gaussian_importance


# ---- the controller -------------------------------------------------------------------------------------------------------------------
if INSIDE_REFERENCE:  # pragma: no cover - only inside the reference repo
    class HipTaming3DGSDensityControllerImpl(VanillaDensityControllerImpl):
        config: HipTaming3DGSDensityController

        def setup(self, stage: str, pl_module) -> None:
            super().setup(stage, pl_module)

            self.register_buffer("_densify_iter_num", torch.tensor(1, dtype=torch.int), persistent=True)

            if stage == "fit":
                start_count = self.config.start_count
                if start_count <= 0:
                    start_count = pl_module.trainer.datamodule.dataparser_outputs.point_cloud.xyz.shape[0]
                self.counts_array = count_array(
                    start_count=start_count,
                    multiplier=self.config.budget,
                    densify_until_iter=self.config.densify_until_iter,
                    densify_from_iter=self.config.densify_from_iter,
                    densification_interval=self.config.densification_interval,
                    mode=self.config.mode,
                )
                print(self.counts_array)

                pl_module.on_train_start_hooks.append(self.on_train_start)

                self.avoid_state_dict = (pl_module,)

        def log_metric(self, name, value):
            self.avoid_state_dict[0].logger.log_metrics({"density/{}".format(name): value}, step=self.avoid_state_dict[0].trainer.global_step)

        def on_train_start(self, gaussian_model, pl_module):
            loader = pl_module.trainer.train_dataloader
            if not hasattr(loader, "max_cache_num") or not hasattr(loader, "cached"):
                raise RuntimeError("HipTaming3DGSDensityController needs the reference's cache dataloader (`max_cache_num`, `cached`): "
                                   f"{type(loader).__name__} has neither")
            assert loader.max_cache_num < 0

            self._densify_iter_num.fill_(max(pl_module.global_step // self.config.densification_interval - self.config.densify_from_iter // self.config.densification_interval, 0) + 1)
            print("densify_iter_num={}, budget={}\n".format(self.densify_iter_num, self.counts_array[self.densify_iter_num]))

            self.all_edges = edge_maps(loader.cached, device=pl_module.device, on_cpu=self.config.edges_on_cpu)

        @property
        def densify_iter_num(self) -> int:
            return self._densify_iter_num.item()

        @densify_iter_num.setter
        def densify_iter_num(self, v):
            self._densify_iter_num.fill_(v)

        def _densify_and_prune(self, max_screen_size, gaussian_model, optimizers: List):
            # calculate mean grads
            grads = self.xyz_gradient_accum / self.denom
            grads[grads.isnan()] = 0.0
            grads = grads.squeeze(-1)

            pl_module = self.avoid_state_dict[0]

            # sample cameras
            n_cameras = len(pl_module.trainer.train_dataloader.cached)
            sample_cameras = []
            sample_edge_losses = []
            for camera_idx in torch.randperm(n_cameras, dtype=torch.int)[:self.config.n_sample_cameras].tolist():
                sample_cameras.append(pl_module.trainer.train_dataloader.cached[camera_idx])
                sample_edge_losses.append(self.all_edges[camera_idx])

            # calculate importance
            gaussian_importance = compute_gaussian_score(
                gaussian_model=gaussian_model,
                renderer=pl_module.renderer,
                global_steps=pl_module.global_step,
                all_grads=grads,
                sample_cameras=sample_cameras,
                edge_losses=sample_edge_losses,
                bg_color=pl_module._fixed_background_color().to(device=pl_module.device),
                score_coeffs=self.config.score_coeffs,
                lambda_dssim=pl_module.metric.config.lambda_dssim,
            )

            self._densify_and_prune_with_scores(grads=grads, scores=gaussian_importance, gaussian_model=gaussian_model, optimizers=optimizers)

            # prune
            self._opacity_culling(gaussian_importance, max_screen_size, gaussian_model, optimizers)

            self.densify_iter_num = self.densify_iter_num + 1

            if torch.cuda.is_available():
                torch.cuda.empty_cache()

        def _densify_and_prune_with_scores(self, grads, scores, gaussian_model, optimizers):
            extent = self.cameras_extent
            scales = gaussian_model.get_scales()
            max_scales = torch.max(scales, dim=-1).values

            grad_qualifiers = grads >= self.config.densify_grad_threshold
            clone_qualifiers = max_scales <= self.config.percent_dense * extent
            split_qualifiers = max_scales > self.config.percent_dense * extent

            all_clones = torch.logical_and(clone_qualifiers, grad_qualifiers)
            all_splits = torch.logical_and(split_qualifiers, grad_qualifiers)
            total_clones = torch.sum(all_clones).item()
            total_splits = torch.sum(all_splits).item()

            curr_points = gaussian_model.n_gaussians
            budget = min(self.counts_array[self.densify_iter_num], total_clones + total_splits + curr_points)
            clone_budget = ((budget - curr_points) * total_clones) // (total_clones + total_splits)
            split_budget = ((budget - curr_points) * total_splits) // (total_clones + total_splits)

            self._densify_and_clone(scores, clone_budget, all_clones, gaussian_model, optimizers)
            self._densify_and_split(scores, split_budget, all_splits, gaussian_model, optimizers)

        def _densify_and_clone(self, scores, budget, filter, gaussian_model, optimizers):
            if budget <= 0:
                return
            scores = scores * filter.float()
            if scores.sum() == 0:
                return
            n_init_points = gaussian_model.n_gaussians
            selected_pts_mask = torch.zeros((n_init_points,), dtype=torch.bool, device=scores.device)

            sampled_indices = torch.multinomial(scores, budget, replacement=False)
            selected_pts_mask[sampled_indices] = True

            # Copy selected Gaussians
            new_properties = {}
            for key, value in gaussian_model.properties.items():
                new_properties[key] = value[selected_pts_mask]

            if self.config.opacity_correction:
                # NEW: Opacity correction
                current_opacity = gaussian_model.get_opacities()[selected_pts_mask]
                alpha_hat = 1. - torch.sqrt(1. - current_opacity)
                raw_alpha_hat = gaussian_model.opacity_inverse_activation(alpha_hat)
                gaussian_model.properties["opacities"][selected_pts_mask] = raw_alpha_hat
                new_properties["opacities"] = raw_alpha_hat

            # Update optimizers and properties
            self._densification_postfix(new_properties, gaussian_model, optimizers)

        def _densify_and_split(self, scores, budget, filter, gaussian_model, optimizers, N: int = 2):
            if budget <= 0:
                return
            scores = scores * filter.float()
            if scores.sum() == 0:
                return
            n_init_points = gaussian_model.n_gaussians

            padded_importance = torch.zeros((n_init_points,), dtype=scores.dtype, device=scores.device)
            padded_importance[:scores.shape[0]] = scores

            selected_pts_mask = torch.zeros_like(padded_importance, dtype=torch.bool, device=scores.device)
            sampled_indices = torch.multinomial(padded_importance, budget, replacement=False)
            selected_pts_mask[sampled_indices] = True

            # Split
            new_properties = self._split_properties(gaussian_model, selected_pts_mask, N)

            # Update optimizers and properties
            self._densification_postfix(new_properties, gaussian_model, optimizers)

            # Prune selected Gaussians, since they are already split
            prune_filter = torch.cat((
                selected_pts_mask,
                torch.zeros(N * selected_pts_mask.sum(), device=scores.device, dtype=torch.bool),
            ))
            self._prune_points(prune_filter, gaussian_model, optimizers)

        def _opacity_culling(self, scores, max_screen_size, gaussian_model, optimizers):
            if self.densify_iter_num >= self.config.cull_opacity_until:
                return

            if self.config.cull_by_max_opacity:
                prune_mask = torch.logical_and(
                    gaussian_model.get_opacity_max() >= 0.,
                    gaussian_model.get_opacity_max() < self.config.cull_opacity_threshold,
                )
                gaussian_model.reset_opacity_max()
            else:
                prune_mask = (gaussian_model.get_opacities() < self.config.cull_opacity_threshold).squeeze()

            max_scales = gaussian_model.get_scales().max(dim=1).values

            # small scale and opacity
            small_scale_mask = max_scales < 1e-4

            if max_screen_size:
                big_points_vs = self.max_radii2D > max_screen_size
                self.log_metric("big_points_vs_count", big_points_vs.sum())
                prune_mask = torch.logical_or(prune_mask, big_points_vs)
                if self.config.cull_big_scale:
                    big_points_ws = max_scales > 0.1 * self.prune_extent
                    self.log_metric("big_points_ws_count", big_points_ws.sum())
                    prune_mask = torch.logical_or(prune_mask, big_points_ws)

            # min altitude
            if self.config.min_alt is not None:
                alt = torch.inner(gaussian_model.get_means(), torch.tensor(self.config.up_direction, dtype=torch.float, device=max_scales.device))
                min_alt_mask = alt < self.config.min_alt
                prune_mask = torch.logical_or(prune_mask, min_alt_mask)
                self.log_metric("min_alt_count", min_alt_mask.sum())

            must_prune_mask = torch.logical_or(prune_mask, small_scale_mask)

            to_remove = torch.sum(prune_mask)
            remove_budget = int(0.5 * to_remove)

            if remove_budget == 0:
                return

            n_init_points = gaussian_model.n_gaussians
            padded_importance = torch.zeros((n_init_points,), dtype=torch.float32)           # on the CPU, as in the reference: so is the draw
            padded_importance[:scores.shape[0]] = 1 / (1e-6 + scores.squeeze())
            selected_pts_mask = torch.zeros_like(padded_importance, dtype=torch.bool, device=scores.device)

            sampled_indices = torch.multinomial(padded_importance, remove_budget, replacement=False)
            selected_pts_mask[sampled_indices] = True
            final_prune = torch.logical_and(prune_mask, selected_pts_mask)
            final_prune = torch.logical_or(final_prune, must_prune_mask)

            self.log_metric("pruned", final_prune.sum())

            self._prune_points(final_prune, gaussian_model, optimizers)

        def update_states(self, outputs):
            viewspace_point_tensor, visibility_filter = outputs["viewspace_points"], outputs["visibility_filter"]
            if self.config.acc_vis:
                visibility_filter = outputs["acc_vis"]
            # retrieve viewspace_points_grad_scale if provided
            viewspace_points_grad_scale = outputs.get("viewspace_points_grad_scale", None)

            # update `max_radii2D` is unnecessary, since it will be reset to 0 after cloning and splitting

            # update states
            xys_grad = viewspace_point_tensor.grad
            if self.config.absgrad is True:
                xys_grad = viewspace_point_tensor.absgrad
            self._add_densification_stats(xys_grad, visibility_filter, scale=viewspace_points_grad_scale)
else:
    HipTaming3DGSDensityControllerImpl = None

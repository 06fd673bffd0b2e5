"""SegAnyGS on the HIP ops: the per-step local feature smoothing of internal/segany_splatting.py:262-309.

The reference computes a K = 16 nearest-neighbour map of the Gaussian centres once (`pytorch3d.ops.knn_points`, :273) and then, every
step, normalises the per-Gaussian features, gathers a random half of each Gaussian's neighbours into an [N, 8, 32] tensor, takes the
mean and normalises again.  `HipFeatureSmoother` does the search with `ops.knn_points`, keeps the map with its inverse adjacency
(`ops.knn_graph`) and runs each step as one `ops.smooth_features` launch per direction.

    module = SegAnySplatting(...)                 # the reference's LightningModule, unedited (compat.install() provides pytorch3d.ops)
    use_hip_smoothing(module)                     # get_processed_semantic_features now runs on the fused op
    use_hip_loss(module)                          # mask_preprocess and forward_with_loss_calculation now run on the section-24 ops

`use_hip_loss` covers what follows the renderer in every step (:152-260, :317-419): the mask statistics, the scale-aware pair labels
and the correspondence loss with its backward (`ops.segany_*`).  It takes the reference's random draws in the reference's order and on
the same devices, so a seeded run consumes the RNG streams identically.
"""
from __future__ import annotations

import types
from typing import Optional

import torch
from torch import Tensor

from . import ops


class HipFeatureSmoother:
    """`get_processed_semantic_features` of the reference as a callable: smoother(features, xyz, training, generator=None) -> [N, D].

    K, dropout: the reference's `smooth_K` and `smooth_dropout`.  In training with 0 < dropout < 1 each call draws
    `torch.randperm(K)[:int(K * dropout)]` (from `generator`, a CPU generator, when given) and averages those columns of the map;
    otherwise all K.  K <= 1 returns the features re-normalised (:265-266, :308).  The neighbour map is computed on the first call
    and again whenever K or the number of points changes; `reset()` drops it (after densification or pruning of a model whose size
    happens to stay the same)."""

    def __init__(self, K: int = 16, dropout: float = 0.5):
        self.K, self.dropout = int(K), float(dropout)
        self.graph: Optional[ops.KnnGraph] = None
        self.last_columns: Optional[Tensor] = None

    def reset(self):
        self.graph = None

    def _map(self, xyz: Tensor) -> "ops.KnnGraph":
        if self.graph is None or self.graph.K != self.K or self.graph.N != xyz.shape[0]:
            with torch.no_grad():
                pts = xyz.detach().to(torch.float32)
                found = ops.knn_points(pts.unsqueeze(0), pts.unsqueeze(0), K=self.K)
                self.graph = ops.knn_graph(found.idx[0])
        return self.graph

    def __call__(self, features: Tensor, xyz: Tensor, training: bool, generator: Optional[torch.Generator] = None) -> Tensor:
        if self.K <= 1:
            return features / (features.norm(dim=-1, keepdim=True) + 1e-9)
        dropout = self.dropout if training else -1.0
        assert dropout < 0 or int(self.K * dropout) >= 1
        columns = None
        if 0 < dropout < 1:
            columns = torch.randperm(self.K, generator=generator)[: int(self.K * dropout)]
        self.last_columns = columns
        return ops.smooth_features(features, self._map(xyz), columns)


def use_hip_smoothing(module, generator: Optional[torch.Generator] = None) -> HipFeatureSmoother:
    """Rebind `get_processed_semantic_features` of a `SegAnySplatting` instance (anything with `gaussian_semantic_features`,
    `models.gaussian.get_xyz`, `smooth_K`, `smooth_dropout` and `training`) to a `HipFeatureSmoother`, which is returned and kept on
    the module as `hip_feature_smoother`.  `smooth_K` and `smooth_dropout` are read at every call, as the reference reads them."""
    smoother = HipFeatureSmoother(getattr(module, "smooth_K", 16), getattr(module, "smooth_dropout", 0.5))

    def get_processed_semantic_features(self):
        smoother.K, smoother.dropout = int(self.smooth_K), float(self.smooth_dropout)
        return smoother(self.gaussian_semantic_features, self.models.gaussian.get_xyz, bool(self.training), generator)

    module.hip_feature_smoother = smoother
    module.get_processed_semantic_features = types.MethodType(get_processed_semantic_features, module)
    return smoother


NUM_SAMPLED_SCALES = 8      # the reference's `num_sampled_scales`; with the upper bound in front and the smallest scale behind: 10


class HipSeganyStep(types.SimpleNamespace):
    """What one `mask_preprocess` on the HIP ops leaves (kept on the module as `hip_segany_step`, with the loss's own draw and selection
    added by `forward_with_loss_calculation`): sampled_ray [H, W] bool, pixel_index [S], a [S] (the mean mask size at the sampled
    pixels), labels [S, S] uint16 and counts [3] (ops.segany_pair_labels), scale_index and upper [Ns] on the device, sampled_scales."""


def _hip_preprocess(self, sam_masks: Tensor, mask_scales: Tensor) -> HipSeganyStep:
    """`mask_preprocess` of the reference up to the point where it would build [N_masks, S] and [S, S] tensors.  The random draws are
    the reference's, in its order and on its devices: randperm(N) and rand(H, W) on the CPU, one rand(1) for the scale in front and one
    per sampled scale.  One host read: the number of sampled pixels."""
    with torch.no_grad():
        device = sam_masks.device
        upper_bound_scale = self.upper_bound_scale
        masks = sam_masks if sam_masks.dtype in (torch.bool, torch.uint8) else sam_masks != 0
        N, H, W = masks.shape
        mask_scales, order = torch.sort(mask_scales.to(device), descending=True)

        picked = torch.randperm(N)[:NUM_SAMPLED_SCALES]
        scale_index = torch.zeros(NUM_SAMPLED_SCALES + 2)
        scale_index[1:len(picked) + 1] = picked
        scale_index[-1] = N - 1
        scale_index[0] = -1
        scale_index = scale_index.long()      # the reference keeps the zeros behind a short randperm as they are
        Ns = scale_index.numel()

        rate = self.ray_sample_rate if self.ray_sample_rate > 0 else self.num_sampled_rays / (H * W)
        sampled_ray = torch.rand(H, W).to(device) < rate
        front = upper_bound_scale + upper_bound_scale * torch.rand(1)[0]
        jitter = torch.stack([torch.rand(1)[0] for _ in range(Ns)]).to(device)

        _, cover, mean_size = ops.segany_mask_stats(masks, order)
        sampled_ray = torch.logical_and(sampled_ray, cover > 0)
        pixel_index = sampled_ray.flatten().nonzero().squeeze(1)      # the step's one host read: S sizes everything below
        S = pixel_index.numel()
        if S < 1:
            raise RuntimeError("use_hip_loss: no pixel was sampled (the reference's max() of an empty tensor raises here as well)")
        if S > ops.segany.MAX_S:
            raise NotImplementedError(f"use_hip_loss: {S} sampled pixels; up to {ops.segany.MAX_S} are built (num_sampled_rays / ray_sample_rate)")

        # the per-scale jitter of the reference's loop, all scales at once and without a branch on a device value
        index = scale_index.to(device)
        scales = mask_scales[index]
        scales[0] = front.to(device)
        upper = scales >= upper_bound_scale
        below = torch.where(mask_scales < upper_bound_scale, mask_scales, torch.full_like(mask_scales, float("-inf")))
        second_big_scale = below.max()
        following = mask_scales[(index + 1).clamp(max=N - 1)]
        last = index == N - 1
        scales = torch.where(upper, scales - (scales - second_big_scale) * jitter,
                             torch.where(last, scales - scales * jitter, scales - (scales - following) * jitter))

        a = mean_size.flatten()[pixel_index]
        bits = ops.segany_pack_membership(masks, order, pixel_index)
        labels, counts = ops.segany_pair_labels(bits, index, upper, n_masks=N)
        sampled_scales = self.q_trans(scales).squeeze()
    return HipSeganyStep(sampled_ray=sampled_ray, pixel_index=pixel_index, a=a, labels=labels, counts=counts, scale_index=index, upper=upper,
                         jittered_scales=scales, sampled_scales=sampled_scales, mask_hw=(H, W))


def pair_weight_matrix(a: Tensor) -> Tensor:
    """The reference's min-max normalised `per_pixel_weight` [S, S] from the mean mask sizes of the sampled pixels, in torch.  The loss
    op forms these values in its kernel; this matrix exists for callers of `mask_preprocess` and for tests."""
    product = a.unsqueeze(0) * a.unsqueeze(1)
    weight = torch.clamp(product.max() / product, 1.0, None)
    return (weight - weight.min()) / (weight.max() - weight.min()) * 9. + 1.


def use_hip_loss(module):
    """Rebind `mask_preprocess` and `forward_with_loss_calculation` of a `SegAnySplatting` instance (anything with `upper_bound_scale`,
    `q_trans`, `ray_sample_rate`, `num_sampled_rays`, `scale_aware_dim`, `scale_gate` or `fixed_scale_gate`, `rfn` and a `forward(camera)`
    that returns {"render": [C, H, W]}) to the ops of include/gspl_hip.h section 24.  Returns the module.

    `forward_with_loss_calculation(camera, image_info, semantic)` returns the reference's tuple
    (rendered_features, loss, cosine_pos, cosine_neg, rendered_feature_norm) with ONE difference: the first element is the renderer's
    map as it came, not that map resampled to the mask size — the resampled map is never made, and `training_step` and
    `validation_step` discard the element.  The norm regulariser stays in torch (one reduce over the map).  The random draws are the
    reference's in its order and on its devices; the [S, S] device draw stands in for `rand_like(sum_0)`.  After the one host read of the
    number of sampled pixels the step has no boolean-mask gather, no `.item()` and no `.cpu()` of its own (`q_trans` is called as the
    module has it).  What the step computed stays on the module as `hip_segany_step`.

    `mask_preprocess(sam_masks, mask_scales)` returns the reference's tuple (sampled_ray, per_pixel_weight, gt_corrs, sampled_scales);
    the two matrices are expanded from the compact results for the caller's sake ([S, S] and [Ns, S, S] float32), which the loss path
    above never does."""

    def mask_preprocess(self, sam_masks, mask_scales):
        step = self.hip_segany_step = _hip_preprocess(self, sam_masks, mask_scales)
        with torch.no_grad():
            shifts = torch.arange(step.upper.numel(), device=step.labels.device, dtype=torch.int32)
            gt_corrs = ((step.labels.to(torch.int32).unsqueeze(0) >> shifts[:, None, None]) & 1).float()
            return step.sampled_ray, pair_weight_matrix(step.a), gt_corrs, step.sampled_scales

    def forward_with_loss_calculation(self, camera, image_info, semantic):
        outputs = self(camera)
        rendered_features = outputs["render"]
        masks, scales = semantic
        step = self.hip_segany_step = _hip_preprocess(self, masks, scales)

        rendered_feature_norm = rendered_features.norm(dim=0, p=2).mean()
        rendered_feature_norm_reg = (1 - rendered_feature_norm) ** 2

        scale_aware_dim = self.scale_aware_dim
        if scale_aware_dim <= 0 or scale_aware_dim >= 32:
            gates = self.scale_gate(step.sampled_scales.unsqueeze(-1))
        else:
            int_sampled_scales = ((1 - step.sampled_scales.squeeze()) * scale_aware_dim).long()
            gates = self.fixed_scale_gate[int_sampled_scales].detach().float()

        S = step.pixel_index.numel()
        step.rand = torch.rand((S, S), dtype=torch.float32, device=rendered_features.device)
        step.gates = gates
        loss, cosine_pos, cosine_neg, step.selected = ops.segany_correspondence_loss(
            rendered_features, step.mask_hw, step.pixel_index, gates, step.labels, step.counts, step.a, step.rand, return_selected=True)
        loss = loss + self.rfn * rendered_feature_norm_reg
        return rendered_features, loss, cosine_pos.detach(), cosine_neg.detach(), rendered_feature_norm

    module.mask_preprocess = types.MethodType(mask_preprocess, module)
    module.forward_with_loss_calculation = types.MethodType(forward_with_loss_calculation, module)
    return module

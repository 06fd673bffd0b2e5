"""The depth-regularisation route (Hierarchical-3DGS style: a monocular depth prior on every training frame) as plugins of the reference's
training loop.

    --model.metric gspl_amd.depthreg.HipHasInverseDepthMetrics        (configs/depth_regularization/*.yaml, *depth_reg*.yaml)
    --model.metric gspl_amd.depthreg.HipDepthMetrics                  (configs/matrixcity/*depth*.yaml)

HipHasInverseDepthMetrics   the reference's `HasInverseDepthMetrics` (internal/metrics/inverse_depth_metrics.py: same fields, defaults, weight
    schedule, logged entries `d_reg` and `d_w`, and `get_predicted_depth` — a batch that carries a depth camera of its own is rendered
    for the depth type alone when the outputs lack it) with the loss from ONE `ops.depth_loss` call: at most two launches forward and
    one backward (csrc/depthloss.hip) where the reference runs six to ten elementwise and reduction launches over [H, W] each way.
    The reference's module imports `torchmetrics` for its `l1+ssim` variant, which is not built here: selecting it raises
    NotImplementedError that says so.
HipDepthMetrics             the reference's `DepthMetrics` (internal/metrics/depth_metrics.py) likewise.
DepthMap                    the reference's `DepthMap` (internal/dataparsers/estimated_depth_colmap_dataparser.py:37-100: `create`, `get`,
    `get_scaled`, `media_normalize`, the uint16 form) without the `cv2` import of its module, so that depth maps can be built and
    read where OpenCV is not installed.  The data parser itself is not restated.

Inside the reference tree the metric bases are the reference's own `VanillaMetrics` / `VanillaMetricsImpl`; stand-alone the classes are
placeholders whose `instantiate` says so, as `gspl_amd.surface.HipGS2DMetrics`.  The arithmetic lives in module-level functions that take
the config, so that it is tested without the reference's classes."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Optional, Union

import numpy as np
import torch

from . import ops

try:  # pragma: no cover - only inside the reference repo
    from internal.metrics.vanilla_metrics import VanillaMetrics as _VanillaMetrics, VanillaMetricsImpl as _VanillaMetricsImpl  # type: ignore
except Exception:
    _VanillaMetrics = _VanillaMetricsImpl = None


@dataclass
class WeightScheduler:
    init: float = 1.0
    final_factor: float = 0.01
    max_steps: int = 30_000


@dataclass
class DepthMap:
    depth: Union[torch.Tensor, np.ndarray]
    scale: Optional[float] = None
    offset: Optional[float] = None
    median: Optional[float] = None
    mask: Optional[torch.Tensor] = None
    camera: Optional[Any] = None

    @classmethod
    def create(cls, depth_map, scale, offset, in_uint16: bool = False):
        """in_uint16: the uint16 map is kept with its scale and offset; otherwise it becomes a float32 tensor, scaled and clamped at 0."""
        if in_uint16:
            assert depth_map.dtype == np.uint16
            return cls(depth=depth_map, scale=scale, offset=offset)
        if depth_map.dtype == np.uint16:
            depth_map = torch.from_numpy(depth_map.astype(np.float32)) / 65535.
        depth_map = depth_map * scale + offset
        depth_map = torch.clamp_min(depth_map, min=0.)
        return cls(depth=depth_map)

    def media_normalize(self):
        """uint16: only the median (of the scaled map's positive values) is taken; otherwise the map is divided by it too."""
        if self.depth.dtype == np.uint16:
            depth = self.get_scaled()
            self.median = torch.median(depth[depth > 0])
        else:
            self.median = torch.median(self.depth[self.depth > 0])
            self.depth = self.depth / self.median

    def get_scaled(self, device="cpu"):
        depth = torch.from_numpy(self.depth.astype(np.float32)).to(device=device) / 65535.
        return (depth * self.scale + self.offset).clamp_min_(min=0.)

    def get(self, device="cpu"):
        if self.depth.dtype == np.uint16:
            depth = self.get_scaled(device=device)
            if self.median is not None:
                depth = depth / self.median
            return depth
        return self.depth.to(device=device)


def check_loss_type(who: str, loss_type: str) -> str:
    """What the reference's `setup` decides: l1 and l2 are built; l1+ssim says why it is not; anything else is NotImplementedError."""
    if loss_type == "l1+ssim":
        raise NotImplementedError(f"{who}: depth_loss_type 'l1+ssim' is not built: the reference takes it from torchmetrics' "
                                  "StructuralSimilarityIndexMeasure (data range from the inputs), which is not available here to pin "
                                  "a restatement against; use 'l1' or 'l2', or the reference's own HasInverseDepthMetrics")
    if loss_type not in ("l1", "l2"):
        raise NotImplementedError(f"{who}: depth_loss_type must be 'l1' or 'l2', got {loss_type!r}")
    return loss_type


def get_weight(config, step: int):
    w = config.depth_loss_weight
    return w.init * (w.final_factor ** min(step / w.max_steps, 1))


def inverse_depth_metric(config, batch, outputs):
    """`HasInverseDepthMetricsModule.get_inverse_depth_metric` on `ops.depth_loss`: the same choice of the normalisation (min / max of the
    prediction, else the data's median, else the mean of the data), the data's mask and the image's mask on both sides."""
    _, image_info, gt = batch
    device = batch[0].device
    if gt is None:
        return torch.tensor(0., device=device)
    normalize, median = None, None
    if config.depth_normalized:
        normalize = "minmax"
    elif gt.median is not None:
        assert config.depth_median_normalization
        normalize, median = "median", gt.median
    elif config.depth_mean_normalization:
        normalize = "mean"
    return ops.depth_loss(outputs[config.depth_output_key].squeeze(0), gt.get(device=device), check_loss_type("HipHasInverseDepthMetrics", config.depth_loss_type),
                          normalize, median, gt_mask=gt.mask, pixel_mask=image_info[-1])


def depth_metric(config, batch, outputs):
    """`DepthMetricsModule.get_inverse_depth_metric` on `ops.depth_loss`: (depth, mask) of the batch, the mask on both sides."""
    camera, _, gt = batch
    if gt is None:
        return torch.tensor(0., device=camera.device)
    gt_depth, gt_mask = gt
    return ops.depth_loss(outputs[config.predicted_depth_key].squeeze(0), gt_depth, check_loss_type("HipDepthMetrics", config.depth_loss_type),
                          gt_mask=gt_mask)


def get_predicted_depth(config, pl_module, gaussian_model, batch, outputs):
    """The outputs, or — when they lack the depth type and the batch's depth map carries a camera — a render of THAT camera for the depth
    type alone (inverse_depth_metrics.py:109-123)."""
    if outputs.get(config.depth_output_key, None) is None and batch[-1] is not None:
        assert batch[-1].camera is not None
        depth_camera = batch[-1].camera.to_device(pl_module.device)
        return pl_module.renderer(depth_camera, gaussian_model, torch.zeros((3,), dtype=torch.float32, device=pl_module.device),
                                  render_types=[config.depth_output_key])
    return outputs


def add_depth_term(basic_metrics, d_reg, weight=None):
    """The entries both reference modules log: `loss` grows by the (weighted) term, `d_reg` is it, `d_w` its weight while training."""
    metrics, pbar = basic_metrics
    if weight is not None:
        d_reg = d_reg * weight
    metrics["loss"] = metrics["loss"] + d_reg
    metrics["d_reg"] = d_reg
    pbar["d_reg"] = True
    if weight is not None:
        metrics["d_w"] = weight
        pbar["d_w"] = True
    return metrics, pbar


_INVERSE_FIELDS = dict(depth_loss_type="l1", depth_loss_ssim_weight=0.2, depth_normalized=False, depth_median_normalization=False,
                       depth_mean_normalization=False, depth_output_key="inverse_depth")

if _VanillaMetrics is not None:
    class HipHasInverseDepthMetricsModule(_VanillaMetricsImpl):
        def setup(self, stage: str, pl_module):
            super().setup(stage, pl_module)
            check_loss_type("HipHasInverseDepthMetrics", self.config.depth_loss_type)

        def get_inverse_depth_metric(self, batch, outputs):
            return inverse_depth_metric(self.config, batch, outputs)

        def get_weight(self, step: int):
            return get_weight(self.config, step)

        def get_predicted_depth(self, pl_module, gaussian_model, batch, outputs):
            return get_predicted_depth(self.config, pl_module, gaussian_model, batch, outputs)

        def get_train_metrics(self, pl_module, gaussian_model, step: int, batch, outputs):
            basic = super().get_train_metrics(pl_module, gaussian_model, step, batch, outputs)
            predicted = self.get_predicted_depth(pl_module, gaussian_model, batch, outputs)
            return add_depth_term(basic, self.get_inverse_depth_metric(batch, predicted), self.get_weight(step))

        def get_validate_metrics(self, pl_module, gaussian_model, batch, outputs):
            basic = super().get_validate_metrics(pl_module, gaussian_model, batch, outputs)
            predicted = self.get_predicted_depth(pl_module, gaussian_model, batch, outputs)
            return add_depth_term(basic, self.get_inverse_depth_metric(batch, predicted))

    @dataclass
    class HipHasInverseDepthMetrics(_VanillaMetrics):
        depth_loss_type: str = "l1"
        depth_loss_ssim_weight: float = 0.2
        depth_loss_weight: WeightScheduler = field(default_factory=lambda: WeightScheduler())
        depth_normalized: bool = False
        depth_median_normalization: bool = False
        depth_mean_normalization: bool = False
        depth_output_key: str = "inverse_depth"

        def instantiate(self, *args, **kwargs):
            return HipHasInverseDepthMetricsModule(self)

    class HipDepthMetricsModule(_VanillaMetricsImpl):
        def setup(self, stage: str, pl_module):
            super().setup(stage, pl_module)
            check_loss_type("HipDepthMetrics", self.config.depth_loss_type)

        def get_inverse_depth_metric(self, batch, outputs):
            return depth_metric(self.config, batch, outputs)

        def get_weight(self, step: int):
            return get_weight(self.config, step)

        def get_train_metrics(self, pl_module, gaussian_model, step: int, batch, outputs):
            basic = super().get_train_metrics(pl_module, gaussian_model, step, batch, outputs)
            return add_depth_term(basic, self.get_inverse_depth_metric(batch, outputs), self.get_weight(step))

        def get_validate_metrics(self, pl_module, gaussian_model, batch, outputs):
            basic = super().get_validate_metrics(pl_module, gaussian_model, batch, outputs)
            return add_depth_term(basic, self.get_inverse_depth_metric(batch, outputs))

    @dataclass
    class HipDepthMetrics(_VanillaMetrics):
        depth_loss_type: str = "l1"
        depth_loss_weight: WeightScheduler = field(default_factory=lambda: WeightScheduler())
        predicted_depth_key: str = "exp_depth"

        def instantiate(self, *args, **kwargs):
            return HipDepthMetricsModule(self)
else:
    @dataclass
    class HipHasInverseDepthMetrics:
        """Stand-alone placeholder: the metric subclasses the reference's `VanillaMetrics` and needs the reference tree."""
        depth_loss_type: str = "l1"
        depth_loss_ssim_weight: float = 0.2
        depth_loss_weight: WeightScheduler = field(default_factory=lambda: WeightScheduler())
        depth_normalized: bool = False
        depth_median_normalization: bool = False
        depth_mean_normalization: bool = False
        depth_output_key: str = "inverse_depth"

        def instantiate(self, *args, **kwargs):
            raise RuntimeError("gspl_amd.depthreg.HipHasInverseDepthMetrics restates internal.metrics.inverse_depth_metrics."
                               "HasInverseDepthMetrics on internal.metrics.vanilla_metrics.VanillaMetrics: run it inside the reference repository")

    @dataclass
    class HipDepthMetrics:
        """Stand-alone placeholder: the metric subclasses the reference's `VanillaMetrics` and needs the reference tree."""
        depth_loss_type: str = "l1"
        depth_loss_weight: WeightScheduler = field(default_factory=lambda: WeightScheduler())
        predicted_depth_key: str = "exp_depth"

        def instantiate(self, *args, **kwargs):
            raise RuntimeError("gspl_amd.depthreg.HipDepthMetrics restates internal.metrics.depth_metrics.DepthMetrics on "
                               "internal.metrics.vanilla_metrics.VanillaMetrics: run it inside the reference repository")

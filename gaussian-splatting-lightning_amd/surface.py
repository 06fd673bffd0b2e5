"""The 2DGS surface regularisers as a plugin of the reference's training loop.

    --model.renderer gspl_amd.renderers.HipVanilla2DGSRenderer --model.renderer.fused_maps true
    --model.metric gspl_amd.surface.HipGS2DMetrics

HipGS2DMetrics   the reference's `GS2DMetrics` (internal/metrics/gs2d_metrics.py: same fields, defaults, schedule and logged entries)
    with the normal-consistency and distortion terms taken from ONE `ops.surface_reg` call — a deterministic two-level reduction
    and one elementwise backward (csrc/normals.hip) instead of a product, a sum over channels, two means and their backward over
    full-resolution maps.  A term whose weight is 0 at the current step is not computed.

Inside the reference tree the bases are the reference's own classes; stand-alone the class is a placeholder that says so, as
`gspl_amd.mcmc.HipMCMCMetrics`."""
from __future__ import annotations

from dataclasses import dataclass

from . import ops

try:  # pragma: no cover - only inside the reference repo
    from internal.metrics.gs2d_metrics import GS2DMetrics as _GS2DMetrics, GS2DMetricsImpl as _GS2DMetricsImpl  # type: ignore
except Exception:
    _GS2DMetrics = _GS2DMetricsImpl = None


def hip_train_metrics(metric, step: int, outputs, basic_metrics):
    """`GS2DMetricsImpl.train_metrics` on `ops.surface_reg`: the same schedule (normal term after step 7000, distortion term after step
    3000), the same two logged entries."""
    metrics, prog_bar = basic_metrics
    lambda_normal = metric.config.lambda_normal if step > 7000 else 0.0
    lambda_dist = metric.config.lambda_dist if step > 3000 else 0.0
    if lambda_normal != 0 or lambda_dist != 0:
        sums = ops.surface_reg(outputs["rend_normal"], outputs["surf_normal"], outputs["rend_dist"] if lambda_dist != 0 else None)
        normal_loss, dist_loss = lambda_normal * sums[0], lambda_dist * sums[1]
    else:
        normal_loss = dist_loss = outputs["rend_dist"].new_zeros(())
    metrics["loss"] = metrics["loss"] + dist_loss + normal_loss
    metrics["normal_loss"] = normal_loss
    prog_bar["normal_loss"] = False
    metrics["dist_loss"] = dist_loss
    prog_bar["dist_loss"] = False
    return metrics, prog_bar


if _GS2DMetrics is not None:
    class HipGS2DMetricsImpl(_GS2DMetricsImpl):
        def train_metrics(self, pl_module, step: int, batch, outputs, basic_metrics):
            return hip_train_metrics(self, step, outputs, basic_metrics)

    @dataclass
    class HipGS2DMetrics(_GS2DMetrics):
        def instantiate(self, *args, **kwargs):
            return HipGS2DMetricsImpl(self)
else:
    @dataclass
    class HipGS2DMetrics:
        """Stand-alone placeholder: the metric subclasses the reference's `GS2DMetrics` and needs the reference tree."""
        lambda_normal: float = 0.05
        lambda_dist: float = 0.

        def instantiate(self, *args, **kwargs):
            raise RuntimeError("gspl_amd.surface.HipGS2DMetrics subclasses internal.metrics.gs2d_metrics.GS2DMetrics: run it inside the "
                               "reference repository")

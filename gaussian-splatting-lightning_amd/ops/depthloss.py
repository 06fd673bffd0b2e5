"""The depth-regularisation loss (`depth_loss`): csrc/depthloss.hip, include/gspl_hip.h section 29.

    depth_loss(pred [H,W], gt [H,W], kind="l1" | "l2", normalize=None | "minmax" | "median" | "mean", median=None,
               gt_mask=None, pixel_mask=None) -> 0-d tensor

What `HasInverseDepthMetricsModule.get_inverse_depth_metric` (internal/metrics/inverse_depth_metrics.py:70-104) and
`DepthMetricsModule.get_inverse_depth_metric` (internal/metrics/depth_metrics.py:52-61) compute, operation by operation:
    minmax   pred = (pred - min pred) / (max pred - min pred + 1e-8), min and max without gradient
    median   pred = pred / median
    mean     gt, pred = gt / mean(gt), pred / mean(gt), the mean taken before the masks
    masks    both sides are multiplied by gt_mask and then by pixel_mask (as the reference does, `pixel_mask.to(torch.uint8)`)
    l1 / l2  mean |gt - pred| / mean (gt - pred)^2 over ALL H W elements, masked ones included
GPU tensors: at most two launches forward (the reduction that minmax / mean need first, then one fused elementwise pass whose sums
have a fixed order: two runs give the same bits), one launch backward, nothing read by the host; a missing kernel is an error.
CPU tensors take the plain-torch restatement, chosen by the inputs' device alone.  The gradient reaches `pred` only.

`l1+ssim` is NOT built: it is torchmetrics' StructuralSimilarityIndexMeasure with its data range taken from the inputs, and there is
no torchmetrics to pin a restatement against."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from .. import _lib as L
from . import _args as A
from ._common import _guarded

KINDS = {"l1": L.GSPL_DEPTH_LOSS_L1, "l2": L.GSPL_DEPTH_LOSS_L2}
NORMS = {None: L.GSPL_DEPTH_NORM_NONE, "minmax": L.GSPL_DEPTH_NORM_MINMAX, "median": L.GSPL_DEPTH_NORM_MEDIAN, "mean": L.GSPL_DEPTH_NORM_MEAN}
_WHO = "depth_loss"


def _check(pred, gt, kind, normalize, median, gt_mask, pixel_mask):
    if kind == "l1+ssim":
        raise NotImplementedError(f"{_WHO}: l1+ssim is not built: it is torchmetrics' StructuralSimilarityIndexMeasure (data range taken "
                                  "from the inputs), and torchmetrics is not available to pin a restatement against; use l1 or l2")
    if kind not in KINDS:
        raise NotImplementedError(f"{_WHO}: kind must be 'l1' or 'l2', got {kind!r}")
    if normalize not in NORMS:
        raise ValueError(f"{_WHO}: normalize must be None, 'minmax', 'median' or 'mean', got {normalize!r}")
    A.shape(_WHO, "pred", A.tensor(_WHO, "pred", pred), ("H", "W"))
    A.shape(_WHO, "gt", A.tensor(_WHO, "gt", gt), tuple(pred.shape))
    if pred.numel() < 1:
        raise ValueError(f"{_WHO}: pred must hold at least one element, got {list(pred.shape)}")
    if (normalize == "median") != (median is not None):
        raise ValueError(f"{_WHO}: `median` goes with normalize='median' (got normalize={normalize!r}, median "
                         f"{'given' if median is not None else 'missing'})")
    for name, m in (("gt_mask", gt_mask), ("pixel_mask", pixel_mask)):
        if m is not None:
            A.numel(_WHO, name, A.tensor(_WHO, name, m), pred.numel())
    for name, t in (("gt", gt), ("gt_mask", gt_mask), ("pixel_mask", pixel_mask)):
        if t is not None and t.device != pred.device:
            raise RuntimeError(f"{_WHO}: {name} is on {t.device}, pred on {pred.device}")


def _depth_loss_torch(pred, gt, kind, normalize, median, gt_mask, pixel_mask):
    """The reference's operations in its order, in the inputs' dtype."""
    if normalize == "minmax":
        with torch.no_grad():
            max_depth, min_depth = pred.max(), pred.min()
        pred = (pred - min_depth) / (max_depth - min_depth + 1e-8)
    elif normalize == "median":
        pred = pred / median
    elif normalize == "mean":
        mean_depth = torch.mean(gt)
        gt, pred = gt / mean_depth, pred / mean_depth
    if gt_mask is not None:
        gt, pred = gt * gt_mask.reshape(gt.shape), pred * gt_mask.reshape(gt.shape)
    if pixel_mask is not None:
        mask = pixel_mask.reshape(gt.shape).to(torch.uint8)
        gt, pred = gt * mask, pred * mask
    return torch.abs(gt - pred).mean() if kind == "l1" else ((gt - pred) ** 2).mean()


def _mask_arg(m: Optional[Tensor], as_uint8: bool):
    """(tensor the kernel reads, its u8 flag): float32 as it is, bytes and bools as bytes; `as_uint8` is the reference's
    `.to(torch.uint8)` of the pixel mask (a truncation for other dtypes)."""
    if m is None:
        return None, 0
    m = m.detach()
    if m.dtype == torch.bool:
        return m.contiguous().view(torch.uint8), 1
    if m.dtype == torch.uint8:
        return m.contiguous(), 1
    if as_uint8:
        return m.to(torch.uint8).contiguous(), 1
    return m.to(torch.float32).contiguous(), 0


class _DepthLossFn(torch.autograd.Function):
    @staticmethod
    @_guarded(1)
    def forward(ctx, pred, gt, kind, normalize, median, gt_mask, pixel_mask):
        p, g = pred.detach().to(torch.float32).contiguous(), gt.detach().to(torch.float32).contiguous()
        H, W = p.shape
        median_dev, median_value = None, 0.0
        if isinstance(median, Tensor) and median.is_cuda:
            median_dev = median.detach().to(device=p.device, dtype=torch.float32).reshape(1).contiguous()
        elif median is not None:
            median_value = float(median)      # (a Python number or a CPU tensor, as the data set's DepthMap keeps it: no device read)
        m1, m1_u8 = _mask_arg(gt_mask, False)
        m2, m2_u8 = _mask_arg(pixel_mask, True)
        nbytes = L.lib().gspl_depth_loss_workspace_bytes(H, W)
        workspace = torch.empty((nbytes,), dtype=torch.uint8, device=p.device)
        out = torch.empty((1,), dtype=torch.float32, device=p.device)
        L.call("gspl_depth_loss_fwd", H, W, KINDS[kind], NORMS[normalize], L.ptr(p), L.ptr(g), L.ptr(median_dev), median_value,
               L.ptr(m1), m1_u8, L.ptr(m2), m2_u8, L.ptr(workspace), nbytes, L.ptr(out), L.stream())
        ctx.save_for_backward(p, g, median_dev, m1, m2, workspace)
        ctx.cfg = (kind, normalize, median_value, m1_u8, m2_u8, pred.dtype)
        return out.reshape(())

    @staticmethod
    @_guarded(0)
    def backward(ctx, grad_out):
        p, g, median_dev, m1, m2, workspace = ctx.saved_tensors
        kind, normalize, median_value, m1_u8, m2_u8, dtype = ctx.cfg
        H, W = p.shape
        v_pred = torch.empty_like(p)
        go = grad_out.detach().to(torch.float32).reshape(1).contiguous()
        L.call("gspl_depth_loss_bwd", H, W, KINDS[kind], NORMS[normalize], L.ptr(p), L.ptr(g), L.ptr(median_dev), median_value,
               L.ptr(m1), m1_u8, L.ptr(m2), m2_u8, L.ptr(workspace), L.ptr(go), L.ptr(v_pred), L.stream())
        return v_pred.to(dtype), None, None, None, None, None, None


def depth_loss(pred: Tensor, gt: Tensor, kind: str = "l1", normalize: Optional[str] = None, median=None,
               gt_mask: Optional[Tensor] = None, pixel_mask: Optional[Tensor] = None) -> Tensor:
    """See the module's docstring.  pred, gt [H, W]; median: a number or a one-element tensor (with normalize='median' only);
    gt_mask, pixel_mask: H W elements each, float32, uint8 or bool (the pixel mask goes through `.to(torch.uint8)` as in the
    reference).  kind='l1+ssim' raises NotImplementedError and says why."""
    _check(pred, gt, kind, normalize, median, gt_mask, pixel_mask)
    if not pred.is_cuda:
        return _depth_loss_torch(pred, gt, kind, normalize, median, gt_mask, pixel_mask)
    return _DepthLossFn.apply(pred, gt, kind, normalize, median, gt_mask, pixel_mask)

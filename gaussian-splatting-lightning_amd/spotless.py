"""The SpotLessSplats (distractor-robust) route as a plugin of the reference's training loop.

    --model.metric gspl_amd.spotless.HipSpotLessMetrics          (configs/spot_less_splats/*.yaml, *-sls-*.yaml)

What `SpotLessMetricsModule` of internal/metrics/spotless_metrics.py spends outside the rasterizer, every training step: a bilinear
resampling of the [1280, 50, 50] Stable-Diffusion feature map to the mask size, a cat with an 80-channel positional encoding, a permute
into a [640 000, 1360] matrix and a small MLP on it; then the error map copied to the host for a 10 000-bin histogram and three
`.item()` reads.  None of it is needed.

The fold.  Bilinear resampling and the first linear layer are both linear, so they commute, and the positional encoding is separable
(its first 40 channels depend on the row only, its last 40 on the column only):
    z[i, j, :] = bilinear(G)[i, j, :] + A[i, :] + B[j, :]
    G = W1[:, :C] sf            at the feature map's own resolution, a [h0 w0, C] @ [C, 16] product
    A = pe_y @ W1[:, C:C+40]^T + b1      [mh, 16]
    B = pe_x @ W1[:, C+40:]^T            [mw, 16]
The three products stay torch matmuls (autograd carries the gradients on to the four parameters); everything per pixel is
`ops.spotless_mask` (csrc/spotless.hip).

Functional core (importable without the reference tree):
  positional_encodings(mh, mw, device) -> (pe_y [mh, 40], pe_x [mw, 40]), cached; `get_positional_encodings` restated operation for
      operation in float32 (the arguments reach 2^19 pi: the float32 rounding of the argument is part of the function).
  fold(module, sf, mh, mw) -> G, A, B, w2, b2
  predict_mask(module, sf, height, width, max_mlp_mask_size) -> (pred_mask_up, pred_mask) in the reference's shapes, on the HIP op.
  predict_mask_torch(...) -> the same fold in plain torch ops on any device and dtype.
  RunningErrorStats: the running error histogram and its three thresholds, kept and updated on the device.

HipSpotLessMetrics / HipSpotLessMetricsImpl: inside the reference tree they subclass `SpotLessMetrics` / `SpotLessMetricsModule` (same
fields, defaults, logged entries, hooks and state-dict names, so checkpoints interchange); stand-alone the class is a placeholder that
says so, as `gspl_amd.surface.HipGS2DMetrics`.

Not built (inherited unchanged from the reference): `cluster: true` (nearest-neighbour cluster voting; its data parser needs
scikit-learn), utils/sd_feature_extraction.py, half precision."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor

from . import ops
from .ops.spotless import _edges      # linspace(0, 1, bins + 1) as torch.histogram and the reference form it (float32, CPU), kept per device

N_FREQ = 20            # the reference's positional encoding of order 20: 40 channels per axis
HIDDEN = 16

try:  # pragma: no cover - only inside the reference repo
    from internal.metrics.spotless_metrics import SpotLessMetrics as _SpotLessMetrics, SpotLessMetricsModule as _SpotLessMetricsModule  # type: ignore
    from internal.metrics.vanilla_metrics import ssim as _ssim  # type: ignore
except Exception:
    _SpotLessMetrics = _SpotLessMetricsModule = _ssim = None

_PE: dict = {}


def axis_coordinate(n: int, device) -> Tensor:
    """index / (n - 1) in float32, formed on `device` as the reference forms it there."""
    return torch.arange(n, device=device) / (n - 1)


def encode_coordinate(coord: Tensor) -> Tensor:
    """[..., 40] = sin | cos of (2^k pi) coord for k < 20, in float32: one axis of `get_positional_encodings(.., 20)`."""
    frequencies = torch.pow(2, torch.arange(N_FREQ, device=coord.device)).float() * torch.pi
    return torch.cat([torch.sin(frequencies * coord[..., None]), torch.cos(frequencies * coord[..., None])], dim=-1)


def _axis_encoding(n: int, device) -> Tensor:
    return encode_coordinate(axis_coordinate(n, device))


def positional_encodings(mh: int, mw: int, device) -> Tuple[Tensor, Tensor]:
    """(pe_y [mh, 40], pe_x [mw, 40]) float32, kept per (mh, mw, device): `get_positional_encodings(mh, mw, 20)[i, j]` is
    cat(pe_y[i], pe_x[j])."""
    if mh < 2 or mw < 2:
        raise ValueError(f"spotless: the mask must be at least 2 x 2 (the reference divides by height - 1), got {(mh, mw)}")
    key = (int(mh), int(mw), str(torch.device(device)))
    if key not in _PE:
        _PE[key] = (_axis_encoding(mh, device), _axis_encoding(mw, device))
    return _PE[key]


def _layers(module):
    first, second = module.mlp[0], module.mlp[2]
    if first.weight.shape[0] != HIDDEN or tuple(second.weight.shape) != (1, HIDDEN):
        raise NotImplementedError(f"spotless: Linear(C + 80, {HIDDEN}) -> ReLU -> Linear({HIDDEN}, 1) is built, got weights "
                                  f"{tuple(first.weight.shape)} and {tuple(second.weight.shape)}")
    return first, second


def fold(module, sf: Tensor, mh: int, mw: int):
    """module with the reference's `mlp.0` / `mlp.2` layers, sf [C, h0, w0] (or [1, C, h0, w0]) -> G [h0, w0, 16], A [mh, 16],
    B [mw, 16], w2 [16], b2 [1] in sf's dtype, by three matmuls."""
    first, second = _layers(module)
    sf = sf[0] if sf.dim() == 4 else sf
    C, h0, w0 = sf.shape
    if first.weight.shape[1] != C + 4 * N_FREQ:
        raise ValueError(f"spotless: the first layer takes {first.weight.shape[1]} features, the map has {C} + {4 * N_FREQ}")
    if min(h0, w0) < 2:
        raise ValueError(f"spotless: the feature map must be at least 2 x 2, got {(h0, w0)}")
    pe_y, pe_x = positional_encodings(mh, mw, sf.device)
    W1 = first.weight
    G = (sf.reshape(C, h0 * w0).t() @ W1[:, :C].t()).reshape(h0, w0, HIDDEN)
    A = pe_y.to(W1.dtype) @ W1[:, C:C + 2 * N_FREQ].t() + first.bias
    B = pe_x.to(W1.dtype) @ W1[:, C + 2 * N_FREQ:].t()
    return G, A, B, second.weight.reshape(HIDDEN), second.bias


def _mask_size(height: int, width: int, max_mlp_mask_size: int):
    resize = max(height, width) > max_mlp_mask_size
    return ((max_mlp_mask_size, max_mlp_mask_size) if resize else (height, width)), resize


def _shaped(mask: Tensor, resize: bool):
    """The [h, w] mask -> (pred_mask_up, pred_mask) as `mlp_mask` returns them: [N, 1] and [1, h, w, 1], or with the second resampling
    the flat [N] and [1, h, w, 1]."""
    pred_mask = mask.reshape(1, mask.shape[0], mask.shape[1], 1)
    return (pred_mask.flatten() if resize else mask.reshape(-1, 1)), pred_mask


def predict_mask(module, sf: Tensor, height: int, width: int, max_mlp_mask_size: int = 800):
    """`SpotLessMetricsModule.mlp_mask`'s prediction on the fused op: (pred_mask_up, pred_mask).  sf [C, h0, w0] or [1, C, h0, w0],
    float32 on the GPU.  With max(height, width) > max_mlp_mask_size the network is evaluated on the square mask of that size and
    resampled to (height, width) in the same launch."""
    (mh, mw), resize = _mask_size(int(height), int(width), int(max_mlp_mask_size))
    G, A, B, w2, b2 = fold(module, sf, mh, mw)
    return _shaped(ops.spotless_mask(G.contiguous(), A, B, w2, b2, out_size=(int(height), int(width)) if resize else None), resize)


def predict_mask_torch(module, sf: Tensor, height: int, width: int, max_mlp_mask_size: int = 800):
    """The same fold in plain torch ops, on any device and in the module's dtype: what the CPU tests pin to the reference and the GPU
    tests compare the op with."""
    (mh, mw), resize = _mask_size(int(height), int(width), int(max_mlp_mask_size))
    G, A, B, w2, b2 = fold(module, sf, mh, mw)
    z = F.interpolate(G.permute(2, 0, 1)[None], size=(mh, mw), mode="bilinear")[0].permute(1, 2, 0) + A[:, None, :] + B[None, :, :]
    mask = torch.sigmoid(torch.relu(z) @ w2 + b2)
    if resize:
        mask = F.interpolate(mask[None, None], size=(int(height), int(width)), mode="bilinear")[0, 0]
    return _shaped(mask, resize)


def running_stats_update(hist: Tensor, counts: Tensor, percentiles: Tensor, edges: Tensor):
    """`update_running_stats` without the host: hist' = 0.95 hist + counts, and for each percentile q the edge at the first index where
    cumsum(hist') reaches sum(hist') q.  -> (hist', thresholds [len(percentiles)]).  No `.cpu()`, `.item()` or boolean-mask indexing."""
    hist = 0.95 * hist + counts.to(hist.dtype)
    cum = torch.cumsum(hist, 0)
    index = torch.searchsorted(cum, torch.sum(hist) * percentiles)      # left: the first index with cum >= target
    return hist, edges[index.clamp_(max=edges.numel() - 1)]


class RunningErrorStats:
    """The running error histogram of the SpotLess route on the device: `hist` [bins], `avg`, `lower`, `upper` (0-d), all device
    tensors, with the reference's initial values."""

    def __init__(self, bins: int = 10000, robust_percentile: float = 0.7, lower_bound: float = 0.5, upper_bound: float = 0.9, device="cuda"):
        self.bins = int(bins)
        self.hist = torch.zeros((self.bins,), dtype=torch.float32, device=device)
        self.avg = torch.tensor(1., dtype=torch.float32, device=device)
        self.lower = torch.tensor(0., dtype=torch.float32, device=device)
        self.upper = torch.tensor(1., dtype=torch.float32, device=device)
        self.percentiles = torch.tensor([robust_percentile, lower_bound, upper_bound], dtype=torch.float32).to(device)
        self.edges = _edges(self.bins, device)

    @property
    def thresholds(self) -> Tensor:
        """[2] (lower, upper): what `ops.spotless_error_stats` takes."""
        return torch.stack([self.lower, self.upper])

    def update(self, counts: Tensor):
        self.hist, picked = running_stats_update(self.hist, counts, self.percentiles, self.edges)
        self.avg, self.lower, self.upper = picked.unbind(0)
        return self


if _SpotLessMetricsModule is not None:
    class HipSpotLessMetricsImpl(_SpotLessMetricsModule):
        COUNTS = "_spotless_counts"

        def _thresholds(self) -> Tensor:
            return torch.stack([self._lower_err, self._upper_err])

        def mlp_mask(self, sf, error_per_pixel, height: int, width: int):
            pred_mask_up, pred_mask = predict_mask(self.spotless_module, sf, height, width, self.config.max_mlp_mask_size)
            return pred_mask_up, pred_mask, self.robust_mask(error_per_pixel, self.lower_err), self.robust_mask(error_per_pixel, self.upper_err)

        def get_train_metrics(self, pl_module, gaussian_model, step: int, batch, outputs):
            if self.config.cluster:
                return super().get_train_metrics(pl_module, gaussian_model, step, batch, outputs)
            camera, image_info, sd_feature = batch
            image_name, gt_image, masked_pixels = image_info
            image = outputs["render"]
            if masked_pixels is not None:
                gt_image = gt_image.clone()
                gt_image[masked_pixels] = image.detach()[masked_pixels]
            H, W = image.shape[1], image.shape[2]
            _, counts, lower_mask, upper_mask = ops.spotless_error_stats(image, gt_image, self._thresholds(), self.config.bin_size)
            # with masked pixels the hook histograms the error against the UNEDITED ground truth: it then takes its own call
            outputs[self.COUNTS] = counts if masked_pixels is None else None
            pred_mask_up, pred_mask = predict_mask(self.spotless_module, sd_feature, H, W, self.config.max_mlp_mask_size)
            raw_pred_mask = pred_mask
            if self.config.schedule is True:
                alpha = np.exp(self.config.schedule_beta * np.floor((1 + step) / 1.5))
                pred_mask = torch.bernoulli(torch.clip(alpha + (1 - alpha) * pred_mask.clone().detach(), min=0.0, max=1.0))
            outputs["pred_mask_up"] = pred_mask_up
            outputs["raw_pred_mask"] = raw_pred_mask
            outputs["pred_mask"] = pred_mask
            outputs["lower_mask"] = lower_mask.reshape(1, H, W, 1)
            outputs["upper_mask"] = upper_mask.reshape(1, H, W, 1)

            per_pixel_error_mask = pred_mask.squeeze(-1).clone().detach()
            rgb_diff_loss = ops.spotless_masked_l1(image, gt_image, per_pixel_error_mask)
            if self.config.lambda_dssim > 0:
                sls_masked_pixels = per_pixel_error_mask * (per_pixel_error_mask > 0.5)
                ssim_metric = _ssim(image * sls_masked_pixels, gt_image * sls_masked_pixels)
            else:
                ssim_metric = 0.
            opacity_reg_loss = 0.
            if self.config.opacity_reg > 0 and step < self.config.densify_until_iter:
                opacity_reg_loss = self.config.opacity_reg * torch.abs(gaussian_model.get_opacity).mean()
            loss = (1.0 - self.lambda_dssim) * rgb_diff_loss + self.lambda_dssim * (1. - ssim_metric) + opacity_reg_loss
            return {"loss": loss, "rgb_diff": rgb_diff_loss, "ssim": ssim_metric, "o_reg": opacity_reg_loss}, \
                   {"loss": True, "rgb_diff": True, "ssim": self.config.lambda_dssim > 0, "o_reg": self.config.opacity_reg > 0}

        def update_running_stats(self, outputs, batch, gaussian_model, step, pl_module):
            if step >= self.config.densify_until_iter:
                return
            counts = outputs.get(self.COUNTS) if isinstance(outputs, dict) else None
            if counts is None:
                counts = ops.spotless_error_stats(outputs["render"].detach(), batch[1][1], self._thresholds(), self.config.bin_size)[1]
            device, cfg = self._hist_err.device, self.config
            key = (cfg.robust_percentile, cfg.lower_bound, cfg.upper_bound, str(device))
            if getattr(self, "_percentiles_key", None) != key:          # uploaded once, not per step
                self._percentiles_key = key
                self._percentiles = torch.tensor(key[:3], dtype=torch.float32).to(device)
            hist, picked = running_stats_update(self._hist_err, counts, self._percentiles, _edges(cfg.bin_size, device))
            self._hist_err.copy_(hist)
            self._avg_err.copy_(picked[0])
            self._lower_err.copy_(picked[1])
            self._upper_err.copy_(picked[2])

    @dataclass
    class HipSpotLessMetrics(_SpotLessMetrics):
        def instantiate(self, *args, **kwargs):
            assert self.rgb_diff_loss == "l1"
            return HipSpotLessMetricsImpl(self)
else:
    @dataclass
    class HipSpotLessMetrics:
        """Stand-alone placeholder: the metric subclasses the reference's `SpotLessMetrics` and needs the reference tree."""
        lower_bound: float = 0.5
        upper_bound: float = 0.9
        bin_size: int = 10000
        cluster: bool = False
        schedule: bool = True
        schedule_beta: float = -3e-3
        reset_sh: int = 8002
        robust_percentile: float = 0.7
        max_mlp_mask_size: int = 800
        opacity_reg: float = 0.
        densify_until_iter: int = 15_000
        n_feature_dims: int = 1280

        def instantiate(self, *args, **kwargs):
            raise RuntimeError("gspl_amd.spotless.HipSpotLessMetrics subclasses internal.metrics.spotless_metrics.SpotLessMetrics: run it "
                               "inside the reference repository")

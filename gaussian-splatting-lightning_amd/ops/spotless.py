"""The SpotLessSplats route outside the rasterizer (internal/metrics/spotless_metrics.py; include/gspl_hip.h section 23,
csrc/spotless.hip).

  spotless_mask(G, A, B, w2, b2, out_size=None) -> the predicted inlier mask [mh, mw], or [H, W] when `out_size` asks for the
      second resampling; differentiable in all five inputs.  The fold that produces G, A and B is in gspl_amd.spotless.
  spotless_error_stats(render, gt, thresholds, bins) -> (err, counts, lower_mask, upper_mask): the per-pixel error, this frame's
      histogram of it and the reference's `robust_mask` at two thresholds, without a host read.
  spotless_masked_l1(render, gt, mask) -> mean(mask[None] |render - gt|), differentiable in `render`.

GPU only, float32; no fallback.  The reference's arithmetic is torch code: the fp64 oracle tests/spotless_oracle.py is pinned to it
through tests/golden/ref_spotless.npz, and the kernels to the oracle."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _lib as L
from . import _args
from ._common import _guarded

HIDDEN = 16
MAX_DIM = 16384
MAX_BINS = 15360

_EDGES: dict = {}


def _mask_shapes(who: str, G: Tensor, A: Tensor, B: Tensor, w2: Tensor, b2: Tensor, out_size):
    """Every check of the mask op's inputs (device, dtype, alignment, shapes) -> h0, w0, mh, mw, H, W as the entry points take them."""
    for name, t in (("G", G), ("A", A), ("B", B), ("w2", w2), ("b2", b2)):
        _args.gpu_tensor(who, name, t, torch.float32, like=None if name == "G" else G, like_name="G")
        if name in ("G", "A", "B"):      # (a non-contiguous table is copied, as ops.hexplane_encode does)
            _args.aligned16(who, name, t)
    if G.dim() != 3 or A.dim() != 2 or B.dim() != 2:
        raise ValueError(f"{who}: G must be [h0, w0, {HIDDEN}], A [mh, {HIDDEN}], B [mw, {HIDDEN}]; got {tuple(G.shape)}, {tuple(A.shape)}, {tuple(B.shape)}")
    widths = {G.shape[2], A.shape[1], B.shape[1], w2.numel()}
    if widths != {HIDDEN}:
        raise NotImplementedError(f"{who}: a hidden width of {HIDDEN} is built (the reference's Linear(.., 16)); got G {G.shape[2]}, A {A.shape[1]}, "
                                  f"B {B.shape[1]}, w2 {w2.numel()}")
    if b2.numel() != 1:
        raise ValueError(f"{who}: b2 must hold one value, got {tuple(b2.shape)}")
    h0, w0, mh, mw = G.shape[0], G.shape[1], A.shape[0], B.shape[0]
    H, W = (0, 0) if out_size is None else (int(out_size[0]), int(out_size[1]))
    dims = [h0, w0, mh, mw] + ([] if out_size is None else [H, W])
    if min(dims) < 2:
        raise ValueError(f"{who}: every map and mask dimension must be at least 2 (the reference divides by height - 1), got {dims}")
    if max(dims) > MAX_DIM:
        raise NotImplementedError(f"{who}: dimensions up to {MAX_DIM} are built, got {dims}")
    if (H, W) == (mh, mw):
        H = W = 0                                           # resampling to the same size is the identity, weights (1, 0)
    return h0, w0, mh, mw, H, W


@_guarded(0)
def spotless_mask_forward(G: Tensor, A: Tensor, B: Tensor, w2: Tensor, b2: Tensor, out_size=None, out: Tensor = None) -> Tensor:
    """The forward launch alone, outside autograd (written into `out` when one is given: contiguous float32 of the result's shape)."""
    h0, w0, mh, mw, H, W = _mask_shapes("spotless_mask", G, A, B, w2, b2, out_size)
    shape = (H, W) if H else (mh, mw)
    out = _args.out("spotless_mask_forward", "out", out, shape, torch.float32, G, contiguous=False)
    L.call("gspl_spotless_mask_fwd", h0, w0, mh, mw, H, W, L.ptr(G, torch.float32), L.ptr(A, torch.float32), L.ptr(B, torch.float32),
           L.ptr(w2, torch.float32), L.ptr(b2, torch.float32), L.ptr(out), L.stream())
    return out


@_guarded(0)
def spotless_mask_backward(G: Tensor, A: Tensor, B: Tensor, w2: Tensor, b2: Tensor, v_out: Tensor, out_size=None,
                           v_G: Tensor = None, v_A: Tensor = None, v_B: Tensor = None, v_w: Tensor = None):
    """The two backward launches alone: v_out in the forward's shape -> (v_G, v_A, v_B, v_w [17] = v_w2 | v_b2), every element written
    (into the caller's buffers where given: contiguous float32 of those shapes)."""
    h0, w0, mh, mw, H, W = _mask_shapes("spotless_mask", G, A, B, w2, b2, out_size)
    shape = (H, W) if H else (mh, mw)
    if not isinstance(v_out, Tensor) or tuple(v_out.shape) != shape or v_out.device != G.device:
        raise ValueError(f"spotless_mask_backward: v_out must be {shape} on {G.device}, got {tuple(v_out.shape)} on {v_out.device}")
    v = v_out.to(torch.float32).contiguous()
    v_G, v_A, v_B, v_w = (_args.out("spotless_mask_backward", name, got, like, torch.float32, G, contiguous=False) for name, got, like in
                          (("v_G", v_G, G.shape), ("v_A", v_A, A.shape), ("v_B", v_B, B.shape), ("v_w", v_w, (HIDDEN + 1,))))
    nbytes = L.lib().gspl_spotless_mask_workspace_bytes(h0, w0, mh, mw)
    workspace = torch.empty((nbytes,), dtype=torch.uint8, device=G.device)
    L.call("gspl_spotless_mask_bwd", h0, w0, mh, mw, H, W, L.ptr(G, torch.float32), L.ptr(A, torch.float32), L.ptr(B, torch.float32),
           L.ptr(w2, torch.float32), L.ptr(b2, torch.float32), L.ptr(v, torch.float32), L.ptr(v_G), L.ptr(v_A), L.ptr(v_B), L.ptr(v_w),
           L.ptr(workspace), nbytes, L.stream())
    return v_G, v_A, v_B, v_w


class _SpotlessMaskFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, G, A, B, w2, b2, out_size):
        saved = [t.detach().contiguous() for t in (G, A, B, w2, b2)]
        ctx.save_for_backward(*saved)
        ctx.out_size, ctx.w2_shape, ctx.b2_shape = out_size, w2.shape, b2.shape
        return spotless_mask_forward(*saved, out_size=out_size)

    @staticmethod
    def backward(ctx, v_out):
        G, A, B, w2, b2 = ctx.saved_tensors
        v_G, v_A, v_B, v_w = spotless_mask_backward(G, A, B, w2, b2, v_out, ctx.out_size)
        return v_G, v_A, v_B, v_w[:HIDDEN].reshape(ctx.w2_shape), v_w[HIDDEN:].reshape(ctx.b2_shape), None


def spotless_mask(G: Tensor, A: Tensor, B: Tensor, w2: Tensor, b2: Tensor, out_size: Optional[Tuple[int, int]] = None) -> Tensor:
    """G [h0, w0, 16] channel-last, A [mh, 16], B [mw, 16], w2 [16] (or [1, 16]), b2 [1]: contiguous float32 on the GPU, G, A and B
    aligned to 16 bytes ->
        sigmoid(b2 + w2 . relu(bilinear(G)[i, j] + A[i] + B[j]))  at every pixel of the mh x mw mask,
    or, with out_size = (H, W), that mask resampled bilinearly to H x W in the same launch (the mask itself is never written).  Both
    resamplings are F.interpolate(mode="bilinear", align_corners=False).  The gradient reaches all five inputs; every sum of the
    backward is taken in a fixed order (two runs give the same bits), hidden activations are recomputed, and pixels whose incoming
    gradient is zero are not evaluated.  A hidden width other than 16 raises NotImplementedError, a dimension below 2 ValueError;
    CPU tensors raise RuntimeError: there is no fallback."""
    _mask_shapes("spotless_mask", G, A, B, w2, b2, out_size)
    return _SpotlessMaskFn.apply(G, A, B, w2, b2, None if out_size is None else (int(out_size[0]), int(out_size[1])))


def _edges(bins: int, device) -> Tensor:
    """linspace(0, 1, bins + 1) as torch.histogram forms its edges (float32, on the CPU), kept on the device per (bins, device)."""
    key = (bins, str(device))
    if key not in _EDGES:
        _EDGES[key] = torch.linspace(0.0, 1.0, bins + 1, dtype=torch.float32).to(device)
    return _EDGES[key]


def _images(who: str, render, gt, *mask):
    """render and gt [3, H, W] (and a mask [H, W] or [1, H, W]): float32 on the GPU, of render's size and on its device."""
    for name, t in (("render", render), ("gt", gt)) + tuple(("mask", m) for m in mask):
        _args.gpu_tensor(who, name, t, torch.float32)
        if name != "mask":
            _args.shape(who, name, t, (3, "H", "W"))
        if t.device != render.device or tuple(t.shape[-2:]) != tuple(render.shape[-2:]):
            raise ValueError(f"{who}: {name} must be {tuple(render.shape[-2:])} on {render.device}, got {tuple(t.shape)} on {t.device}")


@_guarded(0)
def spotless_error_stats(render: Tensor, gt: Tensor, thresholds: Tensor, bins: int, out=None):
    """render, gt [3, H, W] float32 on the GPU, thresholds a float32 DEVICE tensor [2] (lower, upper) ->
        err [H, W]          (|d0| + |d1| + |d2|) / 3
        counts [bins] int32 this frame's histogram of err over (0, 1) with torch.histogram's rules (values outside are dropped)
        lower_mask, upper_mask [H, W] float32: the reference's `robust_mask` (inlier: err < threshold, strictly; 1 where the pixel
                            or at least 5 of the 9 pixels of its zero-padded 3 x 3 neighbourhood are inliers)
    One clear of `counts` and one launch; nothing is read by the host.  No gradient flows through any of the four.  `out`: the four
    buffers to write into (contiguous, of those shapes and dtypes)."""
    who = "spotless_error_stats"
    _images(who, render, gt)
    bins = int(bins)
    if not 1 <= bins <= MAX_BINS:
        raise NotImplementedError(f"{who}: 1 .. {MAX_BINS} bins are built, got {bins}")
    if not isinstance(thresholds, Tensor) or thresholds.device != render.device or thresholds.dtype != torch.float32 or thresholds.numel() != 2:
        raise ValueError(f"{who}: thresholds must be a float32 tensor [2] (lower, upper) on {render.device}")
    H, W = render.shape[1], render.shape[2]
    if H < 1 or W < 1 or max(H, W) > MAX_DIM:
        raise NotImplementedError(f"{who}: H and W must be 1 .. {MAX_DIM}, got {(H, W)}")
    r, g, t = render.detach().contiguous(), gt.detach().contiguous(), thresholds.detach().contiguous()
    if out is None:
        err, lower, upper = (torch.empty((H, W), dtype=torch.float32, device=r.device) for _ in range(3))
        counts = torch.zeros((bins,), dtype=torch.int32, device=r.device)
    else:
        err, counts, lower, upper = out
        for name, got, shape, dtype in (("err", err, (H, W), torch.float32), ("counts", counts, (bins,), torch.int32),
                                        ("lower_mask", lower, (H, W), torch.float32), ("upper_mask", upper, (H, W), torch.float32)):
            _args.buffer(who, f"out's {name}", got, shape, dtype, r, contiguous=False)
        counts.zero_()
    L.call("gspl_spotless_error_stats", H, W, bins, L.ptr(r), L.ptr(g), L.ptr(t), L.ptr(_edges(bins, r.device)), L.ptr(err, torch.float32),
           L.ptr(counts, torch.int32), L.ptr(lower, torch.float32), L.ptr(upper, torch.float32), L.stream())
    return err, counts, lower, upper


def _check_l1(who: str, render, gt, mask):
    _images(who, render, gt, mask)
    if mask.numel() != render.shape[1] * render.shape[2]:
        raise ValueError(f"{who}: mask must be [H, W] or [1, H, W], got {tuple(mask.shape)}")
    if max(render.shape[1:]) > MAX_DIM or min(render.shape[1:]) < 1:
        raise NotImplementedError(f"{who}: H and W must be 1 .. {MAX_DIM}, got {tuple(render.shape[1:])}")


@_guarded(0)
def spotless_masked_l1_forward(render: Tensor, gt: Tensor, mask: Tensor, out: Tensor = None) -> Tensor:
    """The two forward launches alone -> out [1] (written into `out` when one is given).  The inputs are checked as
    `spotless_masked_l1` checks them and must be contiguous."""
    who = "spotless_masked_l1_forward"
    _check_l1(who, render, gt, mask)
    H, W = render.shape[1], render.shape[2]
    out = _args.out(who, "out", out, (1,), torch.float32, render, contiguous=False)
    partials = torch.empty((L.lib().gspl_spotless_l1_partials(H * W),), dtype=torch.float32, device=render.device)
    L.call("gspl_spotless_masked_l1_fwd", H, W, L.ptr(render, torch.float32), L.ptr(gt, torch.float32), L.ptr(mask, torch.float32),
           L.ptr(partials), L.ptr(out, torch.float32), L.stream())
    return out


@_guarded(0)
def spotless_masked_l1_backward(render: Tensor, gt: Tensor, mask: Tensor, grad_out: Tensor, v_render: Tensor = None) -> Tensor:
    """The elementwise backward launch alone: grad_out [1] on the device -> v_render [3, H, W].  Checked as the forward."""
    who = "spotless_masked_l1_backward"
    _check_l1(who, render, gt, mask)
    _args.buffer(who, "grad_out", grad_out, (1,), torch.float32, render, contiguous=False)
    H, W = render.shape[1], render.shape[2]
    v_render = _args.out(who, "v_render", v_render, render.shape, torch.float32, render, contiguous=False)
    L.call("gspl_spotless_masked_l1_bwd", H, W, L.ptr(render, torch.float32), L.ptr(gt, torch.float32), L.ptr(mask, torch.float32),
           L.ptr(grad_out, torch.float32), L.ptr(v_render, torch.float32), L.stream())
    return v_render


class _MaskedL1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, render, gt, mask):
        r, g, m = render.detach().contiguous(), gt.detach().contiguous(), mask.detach().contiguous()
        ctx.save_for_backward(r, g, m)
        return spotless_masked_l1_forward(r, g, m).reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        r, g, m = ctx.saved_tensors
        return spotless_masked_l1_backward(r, g, m, grad_out.to(torch.float32).reshape(1).contiguous()), None, None


def spotless_masked_l1(render: Tensor, gt: Tensor, mask: Tensor) -> Tensor:
    """render, gt [3, H, W], mask [H, W] (or [1, H, W]) float32 on the GPU -> the scalar mean(mask[None] |render - gt|) by a
    deterministic two-level sum.  The backward is elementwise, grad mask sign(render - gt) / (3 H W) with sign(0) = 0; there is no
    gradient for `mask` or `gt`."""
    _check_l1("spotless_masked_l1", render, gt, mask)
    return _MaskedL1Fn.apply(render, gt, mask)

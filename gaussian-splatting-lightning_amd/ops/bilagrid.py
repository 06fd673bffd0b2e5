"""Bilateral-grid slicing and its total-variation loss (Wang et al., "Bilateral Guided Radiance Field Processing"): one C-ABI call
per direction each (include/gspl_hip.h section 14, csrc/bilagrid.hip).

  bilagrid_slice(grids, xy, rgb, grid_idx)   lib_bilagrid's `slice(...)["rgb"]` for 4-D inputs: grids [N, 12, L, GH, GW], xy
      [B or 1, H, W, 2], rgb [B, H, W, 3] and an integer device tensor grid_idx of one element (every image uses it) or B rows
      (image b uses grid_idx[b, 0, ..., 0]).  rgb is read in place when it is interleaved (contiguous) or a channels-last view of
      planar images (`image.permute(1, 2, 0)[None]`); the output has rgb's memory layout.  An index outside [0, N) gives NaN
      rows and adds nothing to the grids' gradient; the index is never read on the host.
  bilagrid_tv(grids)                          lib_bilagrid's `total_variation_loss` on the 5-D grids, a 0-d tensor.

GPU only, float32; no fallback."""
from __future__ import annotations

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from .. import _lib as L
from . import _args as A
from ._args import raw_ptr as _addr
from ._common import _guarded

HWC, CHW = L.GSPL_LAYOUT_HWC, L.GSPL_LAYOUT_CHW


def _image_layout(t: Tensor):
    """(tensor, layout) of a [B, H, W, 3] image: read in place when interleaved or a channels-last view of planar images, else one
    copy to interleaved."""
    if t.is_contiguous():
        return t, HWC
    if t.permute(0, 3, 1, 2).is_contiguous():
        return t, CHW
    return t.contiguous(), HWC


def _empty_image(B: int, H: int, W: int, layout: int, device) -> Tensor:
    if layout == HWC:
        return torch.empty((B, H, W, 3), dtype=torch.float32, device=device)
    return torch.empty((B, 3, H, W), dtype=torch.float32, device=device).permute(0, 2, 3, 1)


def _grid_shape(grids: Tensor):
    if grids.dim() != 5 or grids.shape[1] != 12:
        raise ValueError(f"grids must be [N, 12, L, H, W], got {tuple(grids.shape)}")
    A.contiguous(None, "grids", grids)
    N, _, Lz, GH, GW = (int(s) for s in grids.shape)
    return N, Lz, GH, GW


class _SliceFn(torch.autograd.Function):
    @staticmethod
    @_guarded(0)
    def forward(ctx, grids, xy, rgb, idx, idx_stride):
        N, Lz, GH, GW = _grid_shape(grids)
        B, H, W, _ = rgb.shape
        rgb, layout = _image_layout(rgb)
        out = _empty_image(B, H, W, layout, rgb.device)
        xy_bstride = H * W * 2 if xy.shape[0] > 1 else 0
        L.call("gspl_bilagrid_slice_fwd", N, Lz, GH, GW, B, H, W, L.ptr(grids), L.ptr(xy), xy_bstride, _addr(rgb), layout, L.ptr(idx),
               idx_stride, _addr(out), L.stream())
        ctx.save_for_backward(grids, xy, rgb, idx)
        ctx.cfg = (layout, xy_bstride, idx_stride)
        return out

    @staticmethod
    @once_differentiable
    @_guarded(0)
    def backward(ctx, grad_out):
        grids, xy, rgb, idx = ctx.saved_tensors
        layout, xy_bstride, idx_stride = ctx.cfg
        need_grids, need_rgb = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        if not (need_grids or need_rgb):
            return None, None, None, None, None
        N, Lz, GH, GW = _grid_shape(grids)
        B, H, W, _ = rgb.shape
        go, go_layout = _image_layout(grad_out.float())
        v_grids = torch.empty_like(grids) if need_grids else None
        v_rgb = _empty_image(B, H, W, layout, rgb.device) if need_rgb else None
        ws_bytes = int(L.lib().gspl_bilagrid_workspace_bytes(Lz, GH, GW, B, H, W)) if need_grids else 0
        ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=rgb.device) if need_grids else None
        L.call("gspl_bilagrid_slice_bwd", N, Lz, GH, GW, B, H, W, L.ptr(grids), L.ptr(xy), xy_bstride, _addr(rgb), layout, L.ptr(idx),
               idx_stride, _addr(go), go_layout, L.ptr(v_grids), None if v_rgb is None else _addr(v_rgb), layout, L.ptr(ws), ws_bytes,
               L.stream())
        return v_grids, None, v_rgb, None, None


def bilagrid_slice(grids: Tensor, xy: Tensor, rgb: Tensor, grid_idx: Tensor) -> Tensor:
    """The affine-transformed colours [B, H, W, 3] (header section 14); gradients reach `grids` and `rgb`, never `xy`."""
    for name, t in (("grids", grids), ("xy", xy), ("rgb", rgb)):
        A.gpu_f32("bilateral-grid", name, t)
    if rgb.dim() != 4 or rgb.shape[-1] != 3:
        raise ValueError(f"rgb must be [B, H, W, 3], got {tuple(rgb.shape)}")
    B, H, W, _ = (int(s) for s in rgb.shape)
    if xy.dim() != 4 or xy.shape[-1] != 2 or tuple(xy.shape[1:3]) != (H, W) or xy.shape[0] not in (1, B):
        raise ValueError(f"xy must be [{B} or 1, {H}, {W}, 2] for rgb {tuple(rgb.shape)}, got {tuple(xy.shape)}")
    if xy.requires_grad:
        raise ValueError("xy: the slice gives no gradient to the pixel coordinates (pass it without requires_grad)")
    if not isinstance(grid_idx, Tensor) or grid_idx.dtype.is_floating_point or grid_idx.dtype == torch.bool:
        raise ValueError("grid_idx must be an integer tensor")
    if grid_idx.device != rgb.device:
        grid_idx = grid_idx.to(rgb.device)
    if grid_idx.numel() == 1:
        idx, idx_stride = grid_idx.reshape(1).to(torch.int32), 0
    elif grid_idx.dim() >= 1 and grid_idx.shape[0] == B:
        idx, idx_stride = grid_idx.reshape(B, -1)[:, 0].to(torch.int32).contiguous(), 1
    else:
        raise ValueError(f"grid_idx must hold one index or one row per image ({B}), got shape {tuple(grid_idx.shape)}")
    if grids.device != rgb.device or xy.device != rgb.device:
        raise RuntimeError("grids, xy and rgb must be on one device")
    return _SliceFn.apply(grids, xy.contiguous(), rgb, idx, idx_stride)


class _TvFn(torch.autograd.Function):
    @staticmethod
    @_guarded(0)
    def forward(ctx, x):
        N, C, Lz, GH, GW = (int(s) for s in x.shape)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        partials = torch.empty((L.lib().gspl_bilagrid_tv_partials(x.numel()),), dtype=torch.float32, device=x.device)
        L.call("gspl_bilagrid_tv_fwd", N, C, Lz, GH, GW, L.ptr(x), L.ptr(partials), L.ptr(out), L.stream())
        ctx.save_for_backward(x)
        return out

    @staticmethod
    @once_differentiable
    @_guarded(0)
    def backward(ctx, grad_out):
        x, = ctx.saved_tensors
        N, C, Lz, GH, GW = (int(s) for s in x.shape)
        g = grad_out.float().reshape(1).contiguous()
        v = torch.empty_like(x)
        L.call("gspl_bilagrid_tv_bwd", N, C, Lz, GH, GW, L.ptr(x), L.ptr(g), L.ptr(v), L.stream())
        return v


def bilagrid_tv(x: Tensor) -> Tensor:
    """TV = (1/N) sum_d S_d / K_d of x [N, C, n1, n2, n3] (header section 14), a 0-d tensor with a gradient to x."""
    A.gpu_f32("bilateral-grid", "x", x)
    if x.dim() != 5 or x.numel() == 0:
        raise ValueError(f"x must be a non-empty 5-D tensor [N, C, n1, n2, n3], got {tuple(x.shape)}")
    A.contiguous(None, "x", x)
    return _TvFn.apply(x)

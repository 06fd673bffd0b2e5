"""Wide-feature compositing (`rasterize_features`): many channels per splat over a frozen model, gradient of the features only
(csrc/features.hip; what Feature-3DGS and SegAnyGS ask of a rasterizer)."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from .. import _lib as L
from . import _args as A
from ._common import _guarded, _f32c, _grad_or_zeros
from .binning import LazyLists, bin_gaussians
from .compositing import _composite


class _FeatureFn(torch.autograd.Function):
    """`gspl_feature_fwd` / `gspl_feature_bwd`.  Differentiable inputs: `features` and `backgrounds`; the geometry is detached."""

    @staticmethod
    @_guarded(1)
    def forward(ctx, means2d, conics, features, opacities, backgrounds, width, height, tile_size, offsets, flatten_ids, mode, layout):
        means2d, conics, features, opacities = map(_f32c, (means2d.detach(), conics.detach(), features, opacities.detach()))
        backgrounds = _f32c(backgrounds)
        N, D = features.shape
        dev = means2d.device
        tile_w, tile_h = (width + tile_size - 1) // tile_size, (height + tile_size - 1) // tile_size
        offsets = offsets.to(torch.int32).contiguous()
        assert offsets.numel() == tile_w * tile_h
        lazy = flatten_ids if isinstance(flatten_ids, LazyLists) else None
        if lazy is not None and lazy.settled:
            flatten_ids, lazy = lazy.flat, None
        if lazy is None:
            flatten_ids = flatten_ids.to(torch.int32).contiguous()
            n_isects = flatten_ids.shape[0]
        out = torch.empty((height, width, D) if layout == L.GSPL_LAYOUT_HWC else (D, height, width), dtype=torch.float32, device=dev)
        alphas = torch.empty((height, width), dtype=torch.float32, device=dev)
        final_Ts = torch.empty((height, width), dtype=torch.float32, device=dev)
        last_ids = torch.empty((height, width), dtype=torch.int32, device=dev)

        def launch(n, offs, flat):
            L.call("gspl_feature_fwd", N, n, D, mode, layout, L.ptr(means2d), L.ptr(conics), L.ptr(features), L.ptr(opacities),
                   L.ptr(backgrounds), width, height, tile_size, tile_w, tile_h, L.ptr(offs), L.ptr(flat) if n else None,
                   L.ptr(out), L.ptr(alphas), L.ptr(final_Ts), L.ptr(last_ids), L.stream())

        with torch.cuda.device(dev):
            held = False
            if lazy is not None:
                # the list length is still on the device (LazyLists): composite on the capacity-sized buffer first, look at the count
                # afterwards, and repeat the launch only if the guess had been too low — as _CompositeFn does
                launch(-1, lazy.offsets_ext, lazy.flat_cap)
                held = lazy.settle()
                flatten_ids, offsets = lazy.flat, lazy.offsets.to(torch.int32).contiguous()
                n_isects = flatten_ids.shape[0]
            if not held:
                launch(n_isects, offsets, flatten_ids)
        ctx.save_for_backward(means2d, conics, opacities, offsets, flatten_ids, final_Ts, last_ids)
        ctx.cfg = (N, D, width, height, tile_size, tile_w, tile_h, mode, layout, backgrounds is not None)
        ctx.mark_non_differentiable(alphas)
        return out, alphas

    @staticmethod
    @_guarded(0)
    def backward(ctx, v_out, _v_alphas):
        means2d, conics, opacities, offsets, flatten_ids, final_Ts, last_ids = ctx.saved_tensors
        N, D, width, height, tile_size, tile_w, tile_h, mode, layout, has_bg = ctx.cfg
        dev = means2d.device
        n_isects = flatten_ids.shape[0]
        v_out = _grad_or_zeros(v_out, (height, width, D) if layout == L.GSPL_LAYOUT_HWC else (D, height, width), dev)
        v_features = None
        if ctx.needs_input_grad[2]:
            v_features = torch.zeros((N, D), dtype=torch.float32, device=dev)
            if n_isects > 0 and N > 0:
                L.call("gspl_feature_bwd", N, n_isects, D, mode, layout, L.ptr(means2d), L.ptr(conics), L.ptr(opacities),
                       width, height, tile_size, tile_w, tile_h, L.ptr(offsets), L.ptr(flatten_ids), L.ptr(last_ids),
                       L.ptr(v_out), L.ptr(v_features), L.stream())
        v_bg = None
        if has_bg and ctx.needs_input_grad[4]:
            vo = v_out if layout == L.GSPL_LAYOUT_HWC else v_out.permute(1, 2, 0)
            v_bg = (vo * final_Ts[..., None]).sum(dim=(0, 1))
        return None, None, v_features, None, v_bg, None, None, None, None, None, None, None


def rasterize_features(xys: Tensor, depths: Tensor, radii: Tensor, conics: Tensor, num_tiles_hit: Tensor,
                       features: Tensor, opacity: Tensor, img_height: int, img_width: int, block_width: int,
                       background: Optional[Tensor] = None, return_alpha: bool = False, isects=None, channels_first: bool = False):
    """`rasterize_gaussians` for feature maps: features [N,D], any D >= 1 -> [H,W,D] ([D,H,W] with channels_first), and alpha [H,W]
    when return_alpha.  One binning (or the caller's `isects`), one forward launch, and a backward that computes the gradient of
    `features` (and `background`) and nothing else: the geometry is treated as frozen.  The image is bit-for-bit the one
    `rasterize_gaussians` gives for the same lists.
    When `xys`, `conics` or `opacity` requires a gradient, or the deterministic mode is on (`ops.set_deterministic`: this backward adds
    with atomics in no fixed order), the call is served by `rasterize_gaussians`' own path, unchanged."""
    if block_width not in (8, 16, 32):
        raise NotImplementedError("block_width must be 8, 16 or 32 (the reference default is 16, gsplat_renderer.py:6)")
    if features.dim() != 2 or features.shape[0] != xys.shape[0] or features.shape[1] < 1:
        raise ValueError(f"features must be [N, D] with D >= 1 (got {tuple(features.shape)} for {xys.shape[0]} splats)")
    A.on_gpu(None, "xys", xys, family="gspl")
    A.on_gpu(None, "features", features, family="gspl")
    flat, offsets = isects if isects is not None else bin_gaussians(xys, depths, radii, img_height, img_width, block_width,
                                                                    conics=conics, opacities=opacity, lazy=True)
    layout = L.GSPL_LAYOUT_CHW if channels_first else L.GSPL_LAYOUT_HWC
    geometry_grad = torch.is_grad_enabled() and (xys.requires_grad or conics.requires_grad or opacity.requires_grad)
    if geometry_grad or L.lib().gspl_get_deterministic():
        out, alphas = _composite(xys, conics, features, opacity.reshape(-1), background, img_width, img_height, block_width,
                                 offsets, flat, False, L.GSPL_MODE_GSPLAT, layout)
    else:
        out, alphas = _FeatureFn.apply(xys, conics, features, opacity.reshape(-1), background, img_width, img_height, block_width,
                                       offsets, flat, L.GSPL_MODE_GSPLAT, layout)
    return (out, alphas) if return_alpha else out

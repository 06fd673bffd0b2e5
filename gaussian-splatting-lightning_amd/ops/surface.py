"""Normal maps from depth maps, the 2DGS maps and the surface regulariser sums: one C-ABI call per direction each
(include/gspl_hip.h section 15, csrc/normals.hip).

  depth_to_normal(depth, rays, normalize_rays=False, channels_first=False)
      depth [H, W] (or [1, H, W]), rays a DEVICE [3, 3] matrix A: the normalised cross product of the central differences of
      q(y, x) = depth(y, x) A (x, y, 1)^T, zero on the one-pixel border; [H, W, 3], or [3, H, W] with channels_first.  The gradient
      reaches `depth` only.  `HipVanilla2DGSRenderer.depth_to_normal` and gsplat's `utils.depth_to_normal` are this stencil with two
      different A (`gsplat_rays`).
  surfel_maps(allmap, normal_rot, rays, depth_ratio) -> (rend_normal [3, H, W], surf_depth [1, H, W], surf_normal [3, H, W])
      what the 2DGS renderer derives from the surfel rasterizer's `allmap` [7, H, W], in one launch; the gradient reaches `allmap`.
      One difference from the torch formulation: where alpha is 0 the gradient of planes 0 and 1 is 0, not NaN.
  surface_reg(a, b, dist=None) -> [2]
      (mean(1 - sum_c a_c b_c), mean(dist)) of two [3, H, W] maps and a [H, W] (or [1, H, W]) map: GS2D's normal-consistency and
      distortion terms from one deterministic reduction.

GPU only, float32; no fallback, and no host read-back between the launches."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from .. import _lib as L
from . import _args as A
from ._common import _guarded

HWC, CHW = L.GSPL_LAYOUT_HWC, L.GSPL_LAYOUT_CHW


def _map_hw(t: Tensor, name: str) -> Tuple[Tensor, int, int]:
    """A [H, W] or [1, H, W] map as a contiguous tensor and its size."""
    if t.dim() == 3 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 2:
        raise ValueError(f"{name} must be [H, W] or [1, H, W], got {list(t.shape)}")
    return t.contiguous(), int(t.shape[0]), int(t.shape[1])


class _DepthNormalFn(torch.autograd.Function):
    @staticmethod
    @_guarded(1)
    def forward(ctx, depth, rays, normalize_rays, layout):
        H, W = depth.shape
        out = torch.empty((H, W, 3) if layout == HWC else (3, H, W), dtype=torch.float32, device=depth.device)
        L.call("gspl_depth_normal_fwd", H, W, L.ptr(depth), L.ptr(rays), normalize_rays, layout, L.ptr(out), L.stream())
        ctx.save_for_backward(depth, rays)
        ctx.cfg = (normalize_rays, layout)
        return out

    @staticmethod
    @once_differentiable
    @_guarded(0)
    def backward(ctx, grad_out):
        depth, rays = ctx.saved_tensors
        normalize_rays, layout = ctx.cfg
        H, W = depth.shape
        v = torch.empty_like(depth)
        L.call("gspl_depth_normal_bwd", H, W, L.ptr(depth), L.ptr(rays), normalize_rays, L.ptr(grad_out.float().contiguous()), layout,
               L.ptr(v), L.stream())
        return v, None, None, None


def depth_to_normal(depth: Tensor, rays: Tensor, normalize_rays: bool = False, channels_first: bool = False) -> Tensor:
    """The normal map of `depth` (header section 15): [H, W, 3], or [3, H, W] with channels_first."""
    A.gpu_f32("surface", "depth", depth)
    d, _, _ = _map_hw(depth, "depth")
    return _DepthNormalFn.apply(d, A.gpu_f32("surface", "rays", rays, (3, 3), d, "the maps").detach().contiguous(), int(bool(normalize_rays)), CHW if channels_first else HWC)


def gsplat_rays(camtoworld: Tensor, K: Tensor) -> Tensor:
    """A of gsplat's `utils.depth_to_points` for one image: directions ((x - cx + 0.5) / fx, (y - cy + 0.5) / fy, 1) rotated by
    camtoworld[:3, :3].  Built on the inputs' device; nothing is read back."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    zero, one = torch.zeros_like(fx), torch.ones_like(fx)
    pix = torch.stack([torch.stack([1 / fx, zero, (0.5 - cx) / fx]), torch.stack([zero, 1 / fy, (0.5 - cy) / fy]),
                       torch.stack([zero, zero, one])])
    return camtoworld[:3, :3] @ pix


class _SurfelMapsFn(torch.autograd.Function):
    @staticmethod
    @_guarded(1)
    def forward(ctx, allmap, normal_rot, rays, depth_ratio):
        _, H, W = allmap.shape
        dev = allmap.device
        rend_normal = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        surf_depth = torch.empty((1, H, W), dtype=torch.float32, device=dev)
        surf_normal = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        L.call("gspl_surfel_maps_fwd", H, W, L.ptr(allmap), L.ptr(normal_rot), L.ptr(rays), depth_ratio, L.ptr(rend_normal),
               L.ptr(surf_depth), L.ptr(surf_normal), L.stream())
        ctx.save_for_backward(allmap, normal_rot, rays)
        ctx.depth_ratio = depth_ratio
        return rend_normal, surf_depth, surf_normal

    @staticmethod
    @once_differentiable
    @_guarded(0)
    def backward(ctx, v_rend_normal, v_surf_depth, v_surf_normal):
        allmap, normal_rot, rays = ctx.saved_tensors
        _, H, W = allmap.shape
        grads = [None if g is None else g.float().contiguous() for g in (v_rend_normal, v_surf_depth, v_surf_normal)]
        v_allmap = torch.empty_like(allmap)
        L.call("gspl_surfel_maps_bwd", H, W, L.ptr(allmap), L.ptr(normal_rot), L.ptr(rays), ctx.depth_ratio, L.ptr(grads[0]),
               L.ptr(grads[1]), L.ptr(grads[2]), L.ptr(v_allmap), L.stream())
        return v_allmap, None, None, None


def surfel_maps(allmap: Tensor, normal_rot: Tensor, rays: Tensor, depth_ratio: float) -> Tuple[Tensor, Tensor, Tensor]:
    """(rend_normal, surf_depth, surf_normal) of the surfel rasterizer's allmap [7, H, W] (header section 15): normal_rot [3, 3]
    takes the view-space normal planes to world space, rays [3, 3] is the stencil's A, depth_ratio blends expected and median depth."""
    A.gpu_f32("surface", "allmap", allmap, (7, "H", "W"))
    normal_rot, rays = (A.gpu_f32("surface", name, t, (3, 3), allmap, "the maps").detach().contiguous()
                        for name, t in (("normal_rot", normal_rot), ("rays", rays)))
    return _SurfelMapsFn.apply(allmap.contiguous(), normal_rot, rays, float(depth_ratio))


class _SurfaceRegFn(torch.autograd.Function):
    @staticmethod
    @_guarded(1)
    def forward(ctx, a, b, dist):
        _, H, W = a.shape
        out = torch.empty((2,), dtype=torch.float32, device=a.device)
        partials = torch.empty((2 * L.lib().gspl_surface_reg_partials(H * W),), dtype=torch.float32, device=a.device)
        L.call("gspl_surface_reg_fwd", H, W, L.ptr(a), L.ptr(b), L.ptr(dist), L.ptr(partials), L.ptr(out), L.stream())
        ctx.save_for_backward(a, b)
        ctx.with_dist = dist is not None
        return out

    @staticmethod
    @once_differentiable
    @_guarded(0)
    def backward(ctx, grad_out):
        a, b = ctx.saved_tensors
        _, H, W = a.shape
        need_a, need_b, need_d = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.with_dist and ctx.needs_input_grad[2]
        v_a = torch.empty_like(a) if need_a else None
        v_b = torch.empty_like(b) if need_b else None
        v_d = torch.empty((H, W), dtype=torch.float32, device=a.device) if need_d else None
        if need_a or need_b or need_d:
            L.call("gspl_surface_reg_bwd", H, W, L.ptr(a), L.ptr(b), L.ptr(grad_out.float().contiguous()), L.ptr(v_a), L.ptr(v_b), L.ptr(v_d),
                   L.stream())
        return v_a, v_b, v_d


def surface_reg(a: Tensor, b: Tensor, dist: Optional[Tensor] = None) -> Tensor:
    """out [2] = (mean over pixels of 1 - sum_c a_c b_c, mean of dist; 0 without dist), with gradients to all three (header section 15)."""
    A.gpu_f32("surface", "a", a)
    A.gpu_f32("surface", "b", b)
    if a.dim() != 3 or a.shape[0] != 3 or a.shape != b.shape or a.numel() == 0:
        raise ValueError(f"a and b must be two non-empty [3, H, W] maps, got {list(a.shape)} and {list(b.shape)}")
    if dist is not None:
        A.gpu_f32("surface", "dist", dist)
        dist, H, W = _map_hw(dist, "dist")
        if (H, W) != tuple(a.shape[1:]):
            raise ValueError(f"dist must be [{a.shape[1]}, {a.shape[2]}] (or [1, H, W]), got {[H, W]}")
    return _SurfaceRegFn.apply(a.contiguous(), b.contiguous(), dist)

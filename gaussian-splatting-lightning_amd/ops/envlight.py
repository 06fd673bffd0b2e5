"""Cube-map sampling and the sky blend of the PVG renderer: one C-ABI call per direction each (include/gspl_hip.h section 17,
csrc/envlight.hip).

  cubemap_sample(base, dirs, filter_mode="linear", boundary_mode="cube") -> [..., 3]
      base [6, R, R, 3] (or [1, 6, R, R, 3]) sampled along dirs [..., 3] with seamless bilinear cube filtering: what the reference's
      EnvLight asks of `nvdiffrast.torch.texture`.  These are the published OpenGL / nvdiffrast semantics (the header spells them
      out); parity with nvdiffrast's own build is unpinned.  The gradient reaches `base` alone; directions that require a gradient, a
      texture that is not 3 wide, and other filter or boundary modes are refused.
  envlight_blend(rgb, alpha, base, c2w_rotation, fx, fy, cx, cy, jitter=None, return_dirs=False) -> out [3, H, W] (, dirs [H, W, 3])
      out = rgb + (1 - alpha) sky, the sky sampled along every pixel's ray: d = normalize(((u - cx + ju) / fx, (v - cy + jv) / fy, 1)),
      rotated by c2w_rotation [3, 3] and swapped (x, y, z) -> (x, z, -y) as EnvLight does.  jitter [2, H, W] holds (ju, jv); None
      means pixel centres (0.5).  rgb [3, H, W], alpha [H, W] or [1, H, W].  fx .. cy are python numbers or tensors and go into a
      device table with torch ops; nothing is read back.  Gradients reach rgb, alpha and base.

GPU only, float32; no fallback."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from .. import _lib as L
from . import _args as A
from ._common import _guarded, _f32c


def _texture(base: Tensor) -> Tensor:
    A.tensor(None, "the texture", base)
    if base.dim() == 5 and base.shape[0] == 1:
        base = base[0]
    if base.dim() != 4 or base.shape[0] != 6 or base.shape[1] != base.shape[2] or base.shape[1] < 1:
        raise ValueError(f"the texture must be [6, R, R, 3] (or [1, 6, R, R, 3]), got {list(base.shape)}")
    if base.shape[3] != 3:
        raise NotImplementedError(f"the cube map is built for 3 channels, got {base.shape[3]}")
    return base


class _CubemapFn(torch.autograd.Function):
    @staticmethod
    @_guarded(1)
    def forward(ctx, base, dirs):
        M, R = dirs.shape[0], base.shape[1]
        out = torch.empty((M, 3), dtype=torch.float32, device=base.device)
        L.call("gspl_cubemap_fwd", M, R, L.ptr(dirs), L.ptr(base), L.ptr(out), L.stream())
        ctx.save_for_backward(dirs)
        ctx.R = R
        return out

    @staticmethod
    @once_differentiable
    @_guarded(0)
    def backward(ctx, v_out):
        (dirs,) = ctx.saved_tensors
        R = ctx.R
        g_base = torch.zeros((6, R, R, 3), dtype=torch.float32, device=dirs.device)
        L.call("gspl_cubemap_bwd", dirs.shape[0], R, L.ptr(dirs), L.ptr(_f32c(v_out)), L.ptr(g_base), L.stream())
        return g_base, None


def cubemap_sample(base: Tensor, dirs: Tensor, filter_mode: str = "linear", boundary_mode: str = "cube") -> Tensor:
    """base [6, R, R, 3] sampled along dirs [..., 3] -> [..., 3] (header section 17)."""
    if filter_mode != "linear" or boundary_mode != "cube":
        raise NotImplementedError(f"only filter_mode='linear' with boundary_mode='cube' is built, got {filter_mode!r} / {boundary_mode!r}")
    base = _texture(base)
    if not isinstance(dirs, Tensor) or dirs.dim() < 1 or dirs.shape[-1] != 3:
        raise ValueError(f"the directions must be [..., 3], got {list(getattr(dirs, 'shape', ()))}")
    if dirs.requires_grad:
        raise NotImplementedError("there is no gradient for the directions: detach them")
    A.on_gpu(None, "base", base, family="environment-light")
    A.on_gpu(None, "dirs", dirs, base, "base", family="environment-light")
    out = _CubemapFn.apply(_f32c(base), _f32c(dirs.reshape(-1, 3)))
    return out.view(*dirs.shape[:-1], 3)


def blend_table(c2w_rotation: Tensor, fx, fy, cx, cy, device) -> Tensor:
    """rotation [3, 3] row-major | fx | fy | cx | cy on `device`, built without a read-back."""
    def scalar(v):
        if isinstance(v, Tensor):
            return v.detach().reshape(1).to(device=device, dtype=torch.float32, non_blocking=True)
        return torch.full((1,), float(v), dtype=torch.float32, device=device)      # a fill kernel: no host-to-device copy
    rot = c2w_rotation.detach().to(device=device, dtype=torch.float32).reshape(9)
    return torch.cat([rot, scalar(fx), scalar(fy), scalar(cx), scalar(cy)])


class _BlendFn(torch.autograd.Function):
    @staticmethod
    @_guarded(1)
    def forward(ctx, rgb, alpha, base, table, jitter, return_dirs):
        _, H, W = rgb.shape
        R = base.shape[1]
        out = torch.empty_like(rgb)
        dirs = torch.empty((H, W, 3), dtype=torch.float32, device=rgb.device) if return_dirs else None
        L.call("gspl_envlight_blend_fwd", H, W, R, L.ptr(table), L.ptr(rgb), L.ptr(alpha), L.ptr(base), L.ptr(jitter), L.ptr(out),
               L.ptr(dirs), L.stream())
        ctx.save_for_backward(alpha, base, table, jitter)
        if return_dirs:
            ctx.mark_non_differentiable(dirs)
            return out, dirs
        return out, None

    @staticmethod
    @once_differentiable
    @_guarded(0)
    def backward(ctx, v_out, _v_dirs):
        alpha, base, table, jitter = ctx.saved_tensors
        H, W = alpha.shape[-2:]
        R = base.shape[1]
        v_out = _f32c(v_out)
        need_alpha, need_base = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        g_alpha = torch.empty_like(alpha) if need_alpha else None
        g_base = torch.zeros_like(base) if need_base else None
        if need_alpha or need_base:
            L.call("gspl_envlight_blend_bwd", H, W, R, L.ptr(table), L.ptr(alpha), L.ptr(base), L.ptr(jitter), L.ptr(v_out), L.ptr(g_alpha),
                   L.ptr(g_base), L.stream())
        return (v_out if ctx.needs_input_grad[0] else None), g_alpha, g_base, None, None, None


def envlight_blend(rgb: Tensor, alpha: Tensor, base: Tensor, c2w_rotation: Tensor, fx, fy, cx, cy, jitter: Optional[Tensor] = None,
                   return_dirs: bool = False):
    """rgb + (1 - alpha) sky [3, H, W], the sky sampled along every pixel's ray (header section 17); with return_dirs also the
    float32 directions [H, W, 3] the kernel sampled along."""
    base = _texture(base)
    for t, name in ((rgb, "rgb"), (alpha, "alpha"), (base, "base"), (c2w_rotation, "c2w_rotation")):
        A.on_gpu(None, name, t, family="environment-light")
    if rgb.dim() != 3 or rgb.shape[0] != 3:
        raise ValueError(f"rgb must be [3, H, W], got {list(rgb.shape)}")
    H, W = int(rgb.shape[1]), int(rgb.shape[2])
    if tuple(alpha.shape) not in ((H, W), (1, H, W)):
        raise ValueError(f"alpha must be [{H}, {W}] or [1, {H}, {W}], got {list(alpha.shape)}")
    if tuple(c2w_rotation.shape) != (3, 3):
        raise ValueError(f"c2w_rotation must be [3, 3], got {list(c2w_rotation.shape)}")
    if jitter is not None:
        A.on_gpu(None, "jitter", jitter, family="environment-light")
        if tuple(jitter.shape) != (2, H, W):
            raise ValueError(f"jitter must be [2, {H}, {W}], got {list(jitter.shape)}")
        jitter = _f32c(jitter.detach())
    table = blend_table(c2w_rotation, fx, fy, cx, cy, rgb.device)
    out, dirs = _BlendFn.apply(_f32c(rgb), _f32c(alpha), _f32c(base), table, jitter, bool(return_dirs))
    return (out, dirs) if return_dirs else out

"""The Glossy-Gaussian route's view-dependent opacity (internal/renderers/glossy_renderer.py `get_opacities`,
internal/models/glossy_gaussian.py `get_view_dep_opacities`; include/gspl_hip.h section 25, csrc/glossy.hip).

  sh_view_opacities(degree, means, camera_center, opacity_dc, opacity_rest) -> [N]
      clamp(eval_sh_decomposed(degree, opacity_dc, opacity_rest, normalize(means - camera_center)) + 0.5, 0, 1) in one launch,
      differentiable in opacity_dc and opacity_rest (one launch more).
  sh_view_opacities_forward / sh_view_opacities_backward: the launches alone, outside autograd, into the caller's buffers when given.

GPU only, float32; no fallback.  The reference's arithmetic is torch code: the fp64 oracle tests/glossy_oracle.py is pinned to it
through tests/golden/ref_glossy.npz, and the kernels to the oracle."""
from __future__ import annotations

from typing import Tuple

import torch
from torch import Tensor

from .. import _lib as L
from . import _args as A
from ._common import _guarded, _f32c, _await_updates

MAX_REST = 61          # columns of opacity_rest the kernels stage (the reference's widest row, degree 4, has 24)


def _check(who: str, degree, means, camera_center, dc, rest) -> Tuple[int, int, int]:
    """Every refusal of the op, in `_args`' order for a machine without a GPU: types, shapes and the degree, the dtype, the
    device -> degree, N, Kr.  This runs twice a frame, so each test stands here and `_args` is entered only to refuse."""
    named = (("means", means), ("camera_center", camera_center), ("opacity_dc", dc), ("opacity_rest", rest))
    for name, t in named:
        if not isinstance(t, Tensor):
            A.tensor(who, name, t)
    if means.dim() != 2 or means.shape[1] != 3:
        A.shape(who, "means", means, ("N", 3))
    N = means.shape[0]
    if camera_center.numel() != 3:
        A.numel(who, "camera_center", camera_center, 3)
    if tuple(dc.shape) not in ((N, 1, 1), (N, 1), (N,)):
        raise ValueError(f"{who}: opacity_dc must be [{N}, 1, 1], [{N}, 1] or [{N}], got {tuple(dc.shape)}")
    if rest.dim() not in (2, 3) or rest.shape[0] != N or (rest.dim() == 3 and rest.shape[2] != 1):
        raise ValueError(f"{who}: opacity_rest must be [{N}, Kr, 1] or [{N}, Kr], got {tuple(rest.shape)}")
    Kr = rest.shape[1]
    if int(degree) != degree or not 0 <= degree <= 4:
        raise ValueError(f"{who}: degree must be 0 .. 4, got {degree} (opacity_rest has {Kr} columns)")
    degree = int(degree)
    if Kr < (degree + 1) ** 2 - 1:
        raise ValueError(f"{who}: degree {degree} needs {(degree + 1) ** 2 - 1} columns of opacity_rest, got {Kr}")
    if Kr > MAX_REST:
        raise NotImplementedError(f"{who}: up to {MAX_REST} columns of opacity_rest are built, got {Kr}")
    for name, t in named:
        if t.dtype != torch.float32:
            A.dtype(who, name, t, torch.float32)
    for name, t in named:
        if not t.is_cuda or t.device != means.device:
            A.on_gpu(who, name, t, means, "means")
    return degree, N, Kr


def _operands(degree, means, camera_center, dc, rest, who):
    """The checked inputs as the entry points take them: means [N, 3], origin [3], dc [N], rest [N, Kr]; a contiguous parameter is
    seen in place (a view), anything else is copied (`_f32c` waits for updates in flight before a copy)."""
    degree, N, Kr = _check(who, degree, means, camera_center, dc, rest)
    return degree, N, Kr, _f32c(means.detach()), _f32c(camera_center.detach().reshape(3)), _f32c(dc.reshape(N)), _f32c(rest.reshape(N, Kr))


@_guarded(1)
def sh_view_opacities_forward(degree: int, means: Tensor, camera_center: Tensor, opacity_dc: Tensor, opacity_rest: Tensor,
                              out: Tensor = None) -> Tensor:
    """The forward launch alone, outside autograd -> opacities [N] (written into `out` when one is given: contiguous float32 [N])."""
    who = "sh_view_opacities_forward"
    degree, N, Kr, means, origin, dc, rest = _operands(degree, means, camera_center, opacity_dc, opacity_rest, who)
    out = A.out(who, "out", out, (N,), torch.float32, means)
    _await_updates(opacity_dc, opacity_rest)
    L.call("gspl_sh_opacity_fwd", N, degree, Kr, L.ptr(means), L.ptr(origin), L.ptr(dc), L.ptr(rest) if Kr else None,
           L.ptr(out), L.stream())
    return out


@_guarded(1)
def sh_view_opacities_backward(degree: int, means: Tensor, camera_center: Tensor, opacity_dc: Tensor, opacity_rest: Tensor,
                               v_opacities: Tensor, v_dc: Tensor = None, v_rest: Tensor = None) -> Tuple[Tensor, Tensor]:
    """The backward launch alone: v_opacities [N] -> (v_dc [N], v_rest [N, Kr]), every element written (into the caller's buffers
    where given: contiguous float32 of those shapes)."""
    who = "sh_view_opacities_backward"
    degree, N, Kr, means, origin, dc, rest = _operands(degree, means, camera_center, opacity_dc, opacity_rest, who)
    if not isinstance(v_opacities, Tensor) or v_opacities.numel() != N or v_opacities.device != means.device:
        raise ValueError(f"{who}: v_opacities must hold {N} values on {means.device}")
    v = _f32c(v_opacities.detach().reshape(N))
    v_dc = A.out(who, "v_dc", v_dc, (N,), torch.float32, means)
    v_rest = A.out(who, "v_rest", v_rest, (N, Kr), torch.float32, means)
    _await_updates(opacity_dc, opacity_rest)
    L.call("gspl_sh_opacity_bwd", N, degree, Kr, L.ptr(means), L.ptr(origin), L.ptr(dc), L.ptr(rest) if Kr else None,
           L.ptr(v), L.ptr(v_dc), L.ptr(v_rest) if Kr else None, L.stream())
    return v_dc, v_rest


class _ShOpacityFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, degree, means, origin, dc, rest):
        ctx.save_for_backward(means, origin, dc, rest)
        ctx.degree = degree
        return sh_view_opacities_forward(degree, means, origin, dc, rest)

    @staticmethod
    def backward(ctx, v_opacities):
        means, origin, dc, rest = ctx.saved_tensors
        v_dc, v_rest = sh_view_opacities_backward(ctx.degree, means, origin, dc, rest, v_opacities)
        return None, None, None, v_dc, v_rest


def sh_view_opacities(degree: int, means: Tensor, camera_center: Tensor, opacity_dc: Tensor, opacity_rest: Tensor) -> Tensor:
    """means [N, 3], camera_center [3], opacity_dc [N, 1, 1] ([N, 1], [N]), opacity_rest [N, Kr, 1] ([N, Kr]; Kr may be 0), float32 on
    the GPU ->
        min(max(C0 dc + sum_k basis_k(d) rest[k - 1] + 0.5, 0), 1),   d = (means - camera_center) / max(||means - camera_center||, 1e-12)
    for every row, over the (degree + 1)^2 - 1 first columns of opacity_rest (it may be wider: the colour's active degree rises during
    training while opacity_rest has its full width from the start).  Contiguous parameters are read in place, and an update of them in
    flight on another stream (`FusedAdam(deferred=...)`) is awaited.  The gradient reaches opacity_dc and opacity_rest, in the shapes
    given, where 0 <= the unclamped value <= 1; means and camera_center get none (the reference detaches them).  degree outside
    0 .. 4 or too few columns raise ValueError, another dtype NotImplementedError, CPU tensors RuntimeError: there is no fallback."""
    degree, N, Kr = _check("sh_view_opacities", degree, means, camera_center, opacity_dc, opacity_rest)
    return _ShOpacityFn.apply(degree, means.detach(), camera_center.detach(), opacity_dc.reshape(N), opacity_rest.reshape(N, Kr))

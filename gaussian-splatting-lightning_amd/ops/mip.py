"""The 3D half of the Mip-Splatting route (internal/models/mip_splatting.py: `MipSplattingUtils.compute_3d_filter` :98-162,
`apply_3d_filter_on_scales` :165-180, `apply_3d_filter` :183-200; include/gspl_hip.h section 28, csrc/mip.hip).

  mip_camera_table(cameras, device) -> [C, 16] float32: per camera R (9, row-major), T (3), fx, fy, width, height.  Built once per
      camera set.
  mip_filter_3d(means, camera_table) -> filter_3d [N, 1]: the reference's loop over the cameras, all cameras in one launch (plus one
      for the fill and the two final operations); nothing is read by the host.
  mip_apply_3d_filter(scales, filter_3d, opacities=None, ...) -> (scales_out, opacities_out | coef | None): one launch, one more in
      the backward, optionally with the model's exp / sigmoid activations inside.
  mip_apply_3d_filter_forward / _backward: the launches alone, outside autograd, into the caller's buffers when given.

Where they run: tensors on the GPU go to the HIP kernels, and a missing library is an error, never a torch fallback.  Tensors on the
CPU take the plain-torch restatement below, the reference's own operations in its order (what the CPU tests and
tests/golden/ref_mip.npz exercise, bit for bit); it is chosen by the inputs' device alone.  Mixed devices are refused.

Two documented differences from the reference, both in degenerate input only:
  * when NO Gaussian is valid in any camera the reference raises (`max()` of an empty tensor); here every row keeps the initial
    distance 100000, on either device, and no host read is spent on finding out;
  * the GPU kernels take the opacity coefficient as the product of the three ratios s_i / sqrt(s_i^2 + f^2), not as
    sqrt(prod s_i^2 / prod (s_i^2 + f^2)): in float32 the reference's numerator is subnormal or zero from scales of about 1e-7 on and
    its autograd then returns inf / NaN; the kernels stay finite there, and give coef = 1 exactly where filter_3d is 0.  (The CPU
    restatement keeps the reference's expression, and with it the reference's behaviour.)"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _lib as L
from . import _args as A
from ._common import _guarded, _f32c, _await_updates

CAMERA_FLOATS = L.GSPL_MIP_CAMERA_FLOATS
MAX_N = 2 ** 31 - 1
FAR = 100000.0
SQRT_0_2 = 0.2 ** 0.5


def _camera_row(camera) -> Tensor:
    f = lambda v: torch.as_tensor(v).detach().to(torch.float32).reshape(-1)
    w2c = getattr(camera, "world_to_camera", None)
    R = f(camera.R) if hasattr(camera, "R") else f(w2c[:3, :3].T.contiguous())      # (world_to_camera is stored transposed)
    T = f(camera.T) if hasattr(camera, "T") else f(w2c[3, :3])
    row = [R, T] + [f(getattr(camera, k)) for k in ("fx", "fy", "width", "height")]
    device = R.device
    return torch.cat([t.to(device) for t in row])


def mip_camera_table(cameras: Sequence, device=None) -> Tensor:
    """cameras: objects with `R` [3, 3], `T` [3] (or, without them, `world_to_camera` [4, 4] as the reference stores it, transposed),
    `fx`, `fy`, `width`, `height`, tensors or numbers: the reference's `Camera`, tests/fakes.FakeCamera -> [C, 16] float32 on `device`
    (default: where the first camera's rotation is)."""
    who = "mip_camera_table"
    batched = getattr(cameras, "R", None)
    if isinstance(batched, Tensor) and batched.dim() == 3:                           # the reference's `Cameras`: [C, 3, 3], [C, 3], [C] ...
        C = batched.shape[0]
        if C < 1:
            raise ValueError(f"{who}: at least one camera is needed")
        columns = [getattr(cameras, k).detach().to(device=batched.device, dtype=torch.float32).reshape(C, -1)
                   for k in ("R", "T", "fx", "fy", "width", "height")]
        return torch.cat(columns, dim=1).to(batched.device if device is None else torch.device(device)).contiguous()
    cameras = list(cameras)
    if not cameras:
        raise ValueError(f"{who}: at least one camera is needed")
    rows = [_camera_row(c) for c in cameras]
    for i, r in enumerate(rows):
        if r.numel() != CAMERA_FLOATS:
            raise ValueError(f"{who}: camera {i} gives {r.numel()} values, not 9 + 3 + 4 (R [3, 3], T [3], fx, fy, width, height)")
    device = rows[0].device if device is None else torch.device(device)
    return torch.stack([r.to(device) for r in rows]).contiguous()


# ---- the filter -----------------------------------------------------------------------------------------------------------------------
def _filter_check(who: str, means, table) -> Tuple[int, int]:
    A.tensor(who, "means", means)
    A.tensor(who, "camera_table", table)
    A.shape(who, "means", means, ("N", 3))
    A.shape(who, "camera_table", table, ("C", CAMERA_FLOATS))
    N, C = means.shape[0], table.shape[0]
    if not 1 <= N <= MAX_N:
        raise ValueError(f"{who}: means must hold 1 .. 2^31 - 1 rows, got {N}")
    if C < 1:
        raise ValueError(f"{who}: camera_table must hold at least one camera, got {list(table.shape)}")
    A.dtype(who, "means", means, torch.float32)
    A.dtype(who, "camera_table", table, torch.float32)
    if table.device != means.device:
        raise RuntimeError(f"{who}: camera_table is on {table.device}, means on {means.device}")
    return N, C


def _filter_cpu(means: Tensor, table: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """`compute_3d_filter` operation by operation (the masked assignments as `torch.where`: the same values)."""
    xyz = means
    distance = torch.ones((xyz.shape[0]), device=xyz.device) * FAR
    valid_points = torch.zeros((xyz.shape[0]), device=xyz.device, dtype=torch.bool)
    for row in table:
        R, T = row[:9].reshape(3, 3).T, row[9:12]
        fx, fy, width, height = row[12], row[13], row[14], row[15]
        xyz_cam = xyz @ R + T[None, :]
        valid_depth = xyz_cam[:, 2] > 0.01
        x, y, z = xyz_cam[:, 0], xyz_cam[:, 1], xyz_cam[:, 2]
        z = torch.clamp(z, min=0.001)
        x = x / z * fx + width / 2.0
        y = y / z * fy + height / 2.0
        in_screen = torch.logical_and(torch.logical_and(x >= -0.15 * width, x <= width * 1.15),
                                      torch.logical_and(y >= -0.15 * height, y <= 1.15 * height))
        valid = torch.logical_and(valid_depth, in_screen)
        distance = torch.where(valid, torch.min(distance, z), distance)
        valid_points = torch.logical_or(valid_points, valid)
    focal_length = torch.clamp(table[:, 12].max(), min=0.)
    fill = torch.where(valid_points, distance, torch.zeros_like(distance)).max()      # (all valid distances are > 0.01)
    fill = torch.where(valid_points.any(), fill, torch.full_like(fill, FAR))
    filled = torch.where(valid_points, distance, fill)
    return filled / focal_length * SQRT_0_2, distance, valid_points


@_guarded(0)
def _filter_gpu(means: Tensor, table: Tensor, N: int, C: int, out, want_parts: bool):
    who = "mip_filter_3d"
    means, table = _f32c(means), _f32c(table)
    _await_updates(means)
    out = A.out(who, "out", out, (N, 1), torch.float32, means)
    distance = torch.empty((N,), dtype=torch.float32, device=means.device) if want_parts else None
    valid = torch.empty((N,), dtype=torch.uint8, device=means.device) if want_parts else None
    ws = torch.empty((L.GSPL_MIP_WORKSPACE_BYTES,), dtype=torch.uint8, device=means.device)
    L.call("gspl_mip_filter3d", N, C, L.ptr(means), L.ptr(table), L.ptr(out), L.ptr(distance), L.ptr(valid), L.ptr(ws), L.stream())
    return out, distance, None if valid is None else valid.view(torch.bool)


def mip_filter_3d(means: Tensor, camera_table: Tensor, return_parts: bool = False, out: Optional[Tensor] = None):
    """means [N, 3], camera_table [C, 16] (`mip_camera_table`), float32 on one device -> filter_3d [N, 1] (written into `out` when one
    is given: contiguous float32 [N, 1]); with `return_parts` -> (filter_3d, distance [N], valid_any [N] bool).

    Per Gaussian the smallest clamped depth z over the cameras that see it (p.z > 0.01 and the pixel within 15 % of the image's
    borders, the four comparisons closed), from 100000; a Gaussian no camera sees takes the largest such distance of the others;
    then / the largest fx * sqrt(0.2).  No gradient (the reference computes it under `no_grad`).  When no Gaussian is seen by any
    camera the reference raises; here every row keeps 100000, and nothing is read by the host to find out.
    N == 0 or C == 0 raise ValueError before any launch."""
    who = "mip_filter_3d"
    N, C = _filter_check(who, means, camera_table)
    means, camera_table = means.detach(), camera_table.detach()
    if means.is_cuda:
        filt, distance, valid = _filter_gpu(means, camera_table, N, C, out, bool(return_parts))
    else:
        with torch.no_grad():
            filt, distance, valid = _filter_cpu(means, camera_table)
        filt = filt[..., None]
        if out is not None:
            filt = A.buffer(who, "out", out, (N, 1), torch.float32, means).copy_(filt)
    return (filt, distance, valid) if return_parts else filt


# ---- the application ------------------------------------------------------------------------------------------------------------------
def _apply_check(who: str, scales, filter_3d, opacities, raw_opacities: bool) -> int:
    A.tensor(who, "scales", scales)
    A.tensor(who, "filter_3d", filter_3d)
    if opacities is not None:
        A.tensor(who, "opacities", opacities)
    elif raw_opacities:
        raise TypeError(f"{who}: raw_opacities without opacities")
    A.shape(who, "scales", scales, ("N", 3))
    N = scales.shape[0]
    if N > MAX_N:
        raise ValueError(f"{who}: at most 2^31 - 1 rows, got {N}")
    for name, t in (("filter_3d", filter_3d), ("opacities", opacities)):
        if t is not None and tuple(t.shape) not in ((N, 1), (N,)):
            raise ValueError(f"{who}: {name} must be [{N}, 1] or [{N}], got {list(t.shape)}")
    named = [("scales", scales), ("filter_3d", filter_3d)] + ([("opacities", opacities)] if opacities is not None else [])
    for name, t in named:
        A.dtype(who, name, t, torch.float32)
    for name, t in named[1:]:
        if t.device != scales.device:
            raise RuntimeError(f"{who}: {name} is on {t.device}, scales on {scales.device}")
    return N


def _flags(raw_scales: bool, raw_opacities: bool, compensation: bool) -> int:
    return ((L.GSPL_MIP_RAW_SCALES if raw_scales else 0) | (L.GSPL_MIP_RAW_OPACITIES if raw_opacities else 0)
            | (L.GSPL_MIP_COMPENSATE if compensation else 0))


def _apply_cpu(scales, filter_3d, opacities, raw_scales, raw_opacities, compensation):
    """`apply_3d_filter` / `apply_3d_filter_on_scales`, the reference's operations (differentiable by torch's own autograd)."""
    N = scales.shape[0]
    if raw_scales:
        scales = torch.exp(scales)
    if raw_opacities:
        opacities = torch.sigmoid(opacities)
    scales_square = torch.square(scales)
    scales_after_square = scales_square + torch.square(filter_3d.detach().reshape(N, 1))
    second = opacities
    if compensation:
        det1 = scales_square.prod(dim=1)
        det2 = scales_after_square.prod(dim=1)
        coef = torch.sqrt(det1 / det2)
        second = coef if opacities is None else opacities * coef.reshape((N,) + (1,) * (opacities.dim() - 1))
    return torch.sqrt(scales_after_square), second


@_guarded(0)
def mip_apply_3d_filter_forward(scales: Tensor, filter_3d: Tensor, opacities: Optional[Tensor] = None, *, raw_scales: bool = False,
                                raw_opacities: bool = False, opacity_compensation: bool = True, scales_out: Tensor = None,
                                opacities_out: Tensor = None) -> Tuple[Tensor, Optional[Tensor]]:
    """The forward launch alone, outside autograd, GPU tensors only -> (scales_out [N, 3], opacities_out [N] or None), written into the
    caller's buffers where given (contiguous float32 of those shapes).  The second is o x coef, o (compensation off), coef (no
    opacities), or None (neither)."""
    who = "mip_apply_3d_filter_forward"
    N = _apply_check(who, scales, filter_3d, opacities, raw_opacities)
    A.on_gpu(who, "scales", scales)
    s, f = _f32c(scales.detach()), _f32c(filter_3d.detach().reshape(N))
    o = None if opacities is None else _f32c(opacities.detach().reshape(N))
    scales_out = A.out(who, "scales_out", scales_out, (N, 3), torch.float32, s)
    second = o is not None or opacity_compensation
    if second:
        opacities_out = A.out(who, "opacities_out", opacities_out, (N,), torch.float32, s)
    elif opacities_out is not None:
        raise ValueError(f"{who}: opacities_out without opacities and without opacity_compensation: there is nothing to write")
    _await_updates(scales, opacities)
    L.call("gspl_mip_apply_fwd", N, _flags(raw_scales, raw_opacities, opacity_compensation), L.ptr(s), L.ptr(o), L.ptr(f), L.ptr(scales_out),
           L.ptr(opacities_out) if second else None, L.stream())
    return scales_out, opacities_out if second else None


@_guarded(0)
def mip_apply_3d_filter_backward(scales: Tensor, filter_3d: Tensor, opacities: Optional[Tensor], v_scales_out: Optional[Tensor],
                                 v_opacities_out: Optional[Tensor], *, raw_scales: bool = False, raw_opacities: bool = False,
                                 opacity_compensation: bool = True, want_opacities: bool = True, v_scales: Tensor = None,
                                 v_opacities: Tensor = None) -> Tuple[Tensor, Optional[Tensor]]:
    """The backward launch alone: the gradients of the forward's two outputs ([N, 3] and [N]; None: zero) -> (v_scales [N, 3],
    v_opacities [N] or None), the gradients of the inputs as they were given (raw or activated), every element written."""
    who = "mip_apply_3d_filter_backward"
    N = _apply_check(who, scales, filter_3d, opacities, raw_opacities)
    A.on_gpu(who, "scales", scales)
    s, f = _f32c(scales.detach()), _f32c(filter_3d.detach().reshape(N))
    o = None if opacities is None else _f32c(opacities.detach().reshape(N))
    grads = []
    for name, v, shape in (("v_scales_out", v_scales_out, (N, 3)), ("v_opacities_out", v_opacities_out, (N,))):
        if v is not None:
            if not isinstance(v, Tensor) or v.numel() != N * (3 if len(shape) == 2 else 1) or v.device != s.device:
                raise ValueError(f"{who}: {name} must hold {list(shape)} values on {s.device}")
            v = _f32c(v.detach().reshape(shape))
        grads.append(v)
    if o is None and not opacity_compensation:
        grads[1] = None
    v_scales = A.out(who, "v_scales", v_scales, (N, 3), torch.float32, s)
    if o is not None and want_opacities:
        v_opacities = A.out(who, "v_opacities", v_opacities, (N,), torch.float32, s)
    else:
        v_opacities = None
    _await_updates(scales, opacities)
    L.call("gspl_mip_apply_bwd", N, _flags(raw_scales, raw_opacities, opacity_compensation), L.ptr(s), L.ptr(o), L.ptr(f), L.ptr(grads[0]),
           L.ptr(grads[1]), L.ptr(v_scales), L.ptr(v_opacities), L.stream())
    return v_scales, v_opacities


class _MipApplyFn(torch.autograd.Function):
    """(scales [N, 3], opacities [N] or None, filter_3d [N]) -> (scales_out [N, 3], second [N]); nothing is saved but the inputs."""

    @staticmethod
    def forward(ctx, scales, opacities, filter_3d, raw_scales, raw_opacities, compensation):
        ctx.save_for_backward(scales, filter_3d, *(() if opacities is None else (opacities,)))
        ctx.options = dict(raw_scales=raw_scales, raw_opacities=raw_opacities, opacity_compensation=compensation)
        return mip_apply_3d_filter_forward(scales, filter_3d, opacities, **ctx.options)

    @staticmethod
    def backward(ctx, v_scales_out, v_second):
        scales, filter_3d, *rest = ctx.saved_tensors
        opacities = rest[0] if rest else None
        v_scales, v_opacities = mip_apply_3d_filter_backward(scales, filter_3d, opacities, v_scales_out, v_second,
                                                             want_opacities=opacities is not None and ctx.needs_input_grad[1], **ctx.options)
        return v_scales, v_opacities, None, None, None, None


class _MipScalesFn(torch.autograd.Function):
    """The same with one output: no opacities and no compensation."""

    @staticmethod
    def forward(ctx, scales, filter_3d, raw_scales):
        ctx.save_for_backward(scales, filter_3d)
        ctx.raw_scales = raw_scales
        return mip_apply_3d_filter_forward(scales, filter_3d, None, raw_scales=raw_scales, opacity_compensation=False)[0]

    @staticmethod
    def backward(ctx, v_scales_out):
        scales, filter_3d = ctx.saved_tensors
        return mip_apply_3d_filter_backward(scales, filter_3d, None, v_scales_out, None, raw_scales=ctx.raw_scales, opacity_compensation=False)[0], None, None


def mip_apply_3d_filter(scales: Tensor, filter_3d: Tensor, opacities: Optional[Tensor] = None, *, raw_scales: bool = False,
                        raw_opacities: bool = False, opacity_compensation: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """scales [N, 3], filter_3d [N, 1] ([N]), opacities [N, 1] ([N]) or None, float32 on one device ->

        scales_out = sqrt(s^2 + filter_3d^2)                                  s = exp(scales) with raw_scales, else scales
        coef       = sqrt(prod_i s_i^2 / prod_i (s_i^2 + filter_3d^2))       (opacity_compensation; see the module's note on its form)
        second     = o * coef, in the shape of `opacities`                    o = sigmoid(opacities) with raw_opacities, else opacities
                     o when opacity_compensation is off; coef [N] when there are no opacities; None when neither

    `apply_3d_filter` is (second, scales_out) with opacities, `apply_3d_filter_on_scales` is (scales_out, coef) without.  On the GPU
    one launch, and one more in the backward, which recomputes from the inputs; the gradient reaches `scales` and `opacities` in the
    form they were given, `filter_3d` gets none.  Contiguous parameters are read in place, and an update of them in flight on another
    stream (`FusedAdam(deferred=...)`) is awaited.  CPU tensors take the reference's own torch expression."""
    who = "mip_apply_3d_filter"
    N = _apply_check(who, scales, filter_3d, opacities, raw_opacities)
    raw_scales, raw_opacities, compensation = bool(raw_scales), bool(raw_opacities), bool(opacity_compensation)
    if not scales.is_cuda:
        return _apply_cpu(scales, filter_3d, opacities, raw_scales, raw_opacities, compensation)
    filter_3d = filter_3d.detach().reshape(N)
    if opacities is None and not compensation:
        return _MipScalesFn.apply(scales, filter_3d, raw_scales), None
    if opacities is not None and not compensation and not raw_opacities:      # they pass through: nothing to compute, nothing to copy
        return _MipScalesFn.apply(scales, filter_3d, raw_scales), opacities
    scales_out, second = _MipApplyFn.apply(scales, None if opacities is None else opacities.reshape(N), filter_3d, raw_scales, raw_opacities,
                                           compensation)
    return scales_out, second if opacities is None else second.reshape(opacities.shape)

"""The vibration transform of Periodic Vibration Gaussians: one C-ABI call per direction (include/gspl_hip.h section 17,
csrc/pvg.hip).

  pvg_motion(means, velocity, t, scale_t, opacities, time, cycle, velocity_decay, time_offset=0.0, time_shift=None)
      -> (means_t [N, 3], avg_velocity [N, 3], opacity_t [N, 1])
      what `get_mean_SHM`, `get_marginal_t`, `get_average_velocity` of the reference's model and lines 147-155 of its renderer compute
      with some fifteen elementwise launches: the means at `time + time_offset - time_shift` (moved on by avg_velocity time_shift when
      shifted), the average velocity, and the opacities times the marginal.  t, scale_t and opacities are [N] or [N, 1], scale_t and
      opacities ACTIVATED.  `time` is the camera's time, a python number or a tensor on any device: it goes into a small device table
      with torch ops and is never read back.  Gradients reach the five rows; where the marginal underflows to zero its gradients are
      exactly zero.

GPU only, float32; no fallback, and no host read-back."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from .. import _lib as L
from . import _args as A
from ._common import _guarded, _f32c

_CONSTANTS: dict = {}


def _filled(values, device) -> Tensor:
    """Python numbers as a float32 device tensor, written by fill kernels: no host-to-device copy, so nothing the host waits for."""
    return torch.cat([torch.full((1,), float(v), dtype=torch.float32, device=device) for v in values])


def motion_table(time, time_offset: float, time_shift, cycle: float, velocity_decay: float, device) -> Tensor:
    """The kernel's six scalars on `device`: ts | time_shift | shifted | cycle | velocity_decay | a.  Only the model's constants are
    kept (per device, cycle and velocity_decay); `time_shift`, which training draws anew on every shifted step, and the flag are
    written by fill kernels, and ts = time + time_offset - time_shift is formed from the camera's time with torch ops in float32, in the
    order the reference's renderer forms it.  No step reads anything back or waits for a copy."""
    key = (device, float(cycle), float(velocity_decay))
    const = _CONSTANTS.get(key)
    if const is None:
        if len(_CONSTANTS) > 64:
            _CONSTANTS.clear()
        const = _CONSTANTS[key] = _filled([cycle, velocity_decay, 2.0 * math.pi / float(cycle)], device)
    shift = 0.0 if time_shift is None else float(time_shift)
    if isinstance(time, Tensor):
        ts = time.detach().reshape(1).to(device=device, dtype=torch.float32, non_blocking=True)
    else:
        ts = _filled([time], device)
    ts = ts + float(time_offset)
    if time_shift is not None:
        ts = ts - shift
    return torch.cat([ts, _filled([shift, 1.0 if time_shift is not None else 0.0], device), const])


class _PvgMotionFn(torch.autograd.Function):
    @staticmethod
    @_guarded(1)
    def forward(ctx, means, velocity, t, scale_t, opacities, table):
        N = means.shape[0]
        dev = means.device
        means_t = torch.empty((N, 3), dtype=torch.float32, device=dev)
        avg_velocity = torch.empty((N, 3), dtype=torch.float32, device=dev)
        opacity_t = torch.empty((N, 1), dtype=torch.float32, device=dev)
        L.call("gspl_pvg_motion_fwd", N, L.ptr(means), L.ptr(velocity), L.ptr(t), L.ptr(scale_t), L.ptr(opacities), L.ptr(table),
               L.ptr(means_t), L.ptr(avg_velocity), L.ptr(opacity_t), L.stream())
        ctx.save_for_backward(velocity, t, scale_t, opacities, table)
        return means_t, avg_velocity, opacity_t

    @staticmethod
    @once_differentiable
    @_guarded(0)
    def backward(ctx, v_means_t, v_avg_velocity, v_opacity_t):
        velocity, t, scale_t, opacities, table = ctx.saved_tensors
        N = velocity.shape[0]
        dev = velocity.device
        grads = [_f32c(g) for g in (v_means_t, v_avg_velocity, v_opacity_t)]
        g_means, g_velocity = (torch.empty((N, 3), dtype=torch.float32, device=dev) for _ in range(2))
        g_t, g_scale_t, g_opacities = (torch.empty_like(x) for x in (t, scale_t, opacities))      # each in its own row's shape: [N] or [N, 1]
        L.call("gspl_pvg_motion_bwd", N, L.ptr(velocity), L.ptr(t), L.ptr(scale_t), L.ptr(opacities), L.ptr(table), L.ptr(grads[0]),
               L.ptr(grads[1]), L.ptr(grads[2]), L.ptr(g_means), L.ptr(g_velocity), L.ptr(g_t), L.ptr(g_scale_t), L.ptr(g_opacities),
               L.stream())
        return g_means, g_velocity, g_t, g_scale_t, g_opacities, None


def pvg_motion(means: Tensor, velocity: Tensor, t: Tensor, scale_t: Tensor, opacities: Tensor, time, cycle: float,
               velocity_decay: float = 1.0, time_offset: float = 0.0, time_shift: Optional[float] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """(means_t [N, 3], avg_velocity [N, 3], opacity_t [N, 1]) at the camera time `time` (header section 17)."""
    if not isinstance(means, Tensor) or means.dim() != 2 or means.shape[1] != 3:
        raise ValueError(f"means must be [N, 3], got {list(getattr(means, 'shape', ()))}")
    N = means.shape[0]
    for name, x, width in (("means", means, 3), ("velocity", velocity, 3), ("t", t, 1), ("scale_t", scale_t, 1), ("opacities", opacities, 1)):
        A.on_gpu(None, name, x, family="PVG")
        if x.numel() != N * width or (x.dim() == 2 and x.shape[1] != width) or x.dim() not in (1, 2) or (width == 3 and x.dim() != 2):
            raise ValueError(f"{name} must be [{N}, {width}]" + (f" or [{N}]" if width == 1 else "") + f", got {list(x.shape)}")
    if not float(cycle) > 0:
        raise ValueError(f"cycle must be positive, got {cycle}")
    table = motion_table(time, time_offset, time_shift, cycle, velocity_decay, means.device)
    # ([N] rows come back as [N] gradients, [N, 1] rows as [N, 1]: the autograd function keeps the shape it was given)
    return _PvgMotionFn.apply(_f32c(means), _f32c(velocity), *[_f32c(x) for x in (t, scale_t, opacities)], table)

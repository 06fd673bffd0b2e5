"""The HexPlane / K-Planes field: the ONE primitive in front of the rasterizer that the 4D-GS route needs
(internal/model_components/gs4d_hexplane.py `HexPlaneField`; include/gspl_hip.h section 22, csrc/hexplane.hip).

  hexplane_layout(resolution, multires, F) -> HexPlaneLayout: per level and plane (a, b, R_a, R_b, offset) and the totals, pure
      numpy, usable on the CPU.
  hexplane_pack(planes, layout) -> the flat channel-last table [total, F] from the reference-shaped parameters (L lists of six
      [1, F, R_b, R_a] tensors); plain differentiable torch, so gradients reach the parameters.
  hexplane_encode(x, t, table, aabb, layout) -> [N, L * F]; differentiable in `table`, and in `x` when x requires a gradient.
  hexplane_forward / hexplane_backward: the launches alone, outside autograd, into the caller's buffers.

GPU only, float32; no fallback.  The reference's arithmetic is torch code: the fp64 oracle tests/hexplane_oracle.py is pinned to it
through tests/golden/ref_hexplane.npz, and the kernels to the oracle."""
from __future__ import annotations

import itertools
from dataclasses import dataclass
from typing import Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from .. import _lib as L
from . import _args as A
from ._args import host_ptr as _host
from ._common import _guarded

MAX_LEVELS = 8
FEATURES = (8, 16, 32, 64)
MAX_RESOLUTION = 32768
PLANES = tuple(itertools.combinations(range(4), 2))      # xy, xz, xt, yz, yt, zt: axis a runs along the width


@dataclass(frozen=True)
class HexPlaneLayout:
    """The level / plane table of a HexPlane field.  resolutions [L, 4] uint32 (R_x, R_y, R_z, R_t per level: the multiplier applies to
    the spatial axes only), offsets [6 L + 1] uint32 (first row of plane p of level l at [6 l + p]; offsets[-1] == total), planes: per
    level six tuples (a, b, R_a, R_b, offset).  The parameter of a plane is [1, F, R_b, R_a]; the table has `total` rows of F floats."""
    n_levels: int
    n_features: int
    resolutions: np.ndarray
    offsets: np.ndarray
    planes: Tuple[Tuple[Tuple[int, int, int, int, int], ...], ...]
    total: int

    @property
    def n_output_dims(self) -> int:
        return self.n_levels * self.n_features

    @property
    def n_params(self) -> int:
        return self.total * self.n_features

    def plane_shape(self, level: int, plane: int) -> Tuple[int, int, int, int]:
        a, b, Ra, Rb, _ = self.planes[level][plane]
        return (1, self.n_features, Rb, Ra)


def hexplane_layout(resolution: Sequence[int], multires: Sequence[int], F: int) -> HexPlaneLayout:
    """resolution [r_x, r_y, r_z, r_t] and the level multipliers (the reference's `kplanes_config["resolution"]` and `multires`), F the
    features per plane (`output_coordinate_dim`).  Level l has [r_x m_l, r_y m_l, r_z m_l, r_t]."""
    resolution, multires, F = [int(r) for r in resolution], [int(m) for m in multires], int(F)
    if len(resolution) != 4:
        raise NotImplementedError(f"hexplane_layout: resolution must have 4 entries (input_coordinate_dim 4 is built), got {len(resolution)}")
    if not 1 <= len(multires) <= MAX_LEVELS:
        raise NotImplementedError(f"hexplane_layout: multires must have 1 .. {MAX_LEVELS} levels, got {len(multires)}")
    if F not in FEATURES:
        raise NotImplementedError(f"hexplane_layout: F (output_coordinate_dim) must be one of {FEATURES}, got {F}")
    levels, planes, offsets, at = [], [], [0], 0
    for m in multires:
        res = [r * m for r in resolution[:3]] + resolution[3:]
        if min(res) < 1 or max(res) > MAX_RESOLUTION:
            raise ValueError(f"hexplane_layout: every resolution must be 1 .. {MAX_RESOLUTION}, got {res} (multires {m})")
        levels.append(res)
        row = []
        for a, b in PLANES:
            row.append((a, b, res[a], res[b], at))
            at += res[a] * res[b]
            offsets.append(at)
        planes.append(tuple(row))
    if at >= 2 ** 31:
        raise ValueError(f"hexplane_layout: the table would have {at} rows; fewer than 2^31 are built")
    return HexPlaneLayout(len(multires), F, np.asarray(levels, dtype=np.uint32), np.asarray(offsets, dtype=np.uint32), tuple(planes), at)


def hexplane_pack(planes, layout: HexPlaneLayout) -> Tensor:
    """The reference-shaped parameters (`HexPlaneField.grids`: L lists of six [1, F, R_b, R_a] tensors) -> the flat channel-last table
    [total, F].  Plain torch (a permute and a cat): the gradient of the table reaches every parameter."""
    if len(planes) != layout.n_levels:
        raise ValueError(f"hexplane_pack: {layout.n_levels} levels expected, got {len(planes)}")
    rows = []
    for level, grids in enumerate(planes):
        if len(grids) != 6:
            raise ValueError(f"hexplane_pack: level {level} must have six planes, got {len(grids)}")
        for plane, grid in enumerate(grids):
            if tuple(grid.shape) != layout.plane_shape(level, plane):
                raise ValueError(f"hexplane_pack: plane {plane} of level {level} must be {layout.plane_shape(level, plane)}, got {tuple(grid.shape)}")
            rows.append(grid[0].permute(1, 2, 0).reshape(-1, layout.n_features))
    return torch.cat(rows, dim=0)


def hexplane_box(aabb) -> np.ndarray:
    """aabb [2, 3] (the reference keeps the MAXIMUM corner in aabb[0]) -> the host array [6] the kernels take: aabb[0], then
    float32(2 / (aabb[1] - aabb[0])), both operations in float32 as `normalize_aabb` does them.  A tensor on the GPU is read back:
    keep the result where the box does not change."""
    if isinstance(aabb, Tensor):
        aabb = aabb.detach().cpu().numpy()
    aabb = np.asarray(aabb, dtype=np.float32)
    if aabb.shape == (6,):
        return np.ascontiguousarray(aabb)
    if aabb.shape != (2, 3):
        raise ValueError(f"hexplane: aabb must be [2, 3], got {aabb.shape}")
    with np.errstate(divide="ignore"):
        scale = np.float32(2.0) / (aabb[1] - aabb[0])
    return np.ascontiguousarray(np.concatenate([aabb[0], scale]).astype(np.float32))


def _time(t, x: Tensor):
    """t -> (device pointer or None, the uniform value): a python number is ONE time for the call, a tensor [N] / [N, 1] one per point."""
    if isinstance(t, Tensor):
        if t.numel() != x.shape[0] or t.device != x.device or t.dtype != torch.float32:
            raise ValueError(f"hexplane: t must be a number or float32 [{x.shape[0]}] on {x.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        return t.detach().reshape(-1).contiguous(), 0.0
    return None, float(t)


@_guarded(0)
def hexplane_forward(x: Tensor, t: Union[float, Tensor], table: Tensor, box: np.ndarray, layout: HexPlaneLayout, out: Tensor = None) -> Tensor:
    """The forward launch alone, outside autograd: x [N, 3] and table contiguous float32 on the GPU, box from `hexplane_box` -> out
    [N, L * F] (written into `out` when one is given: contiguous float32 of that shape, 16-byte aligned)."""
    lv, N = layout, x.shape[0]
    if out is None:
        out = torch.empty((N, lv.n_output_dims), dtype=torch.float32, device=x.device)
    else:
        A.buffer("hexplane_forward", "out", out, (N, lv.n_output_dims), torch.float32, x, contiguous=False)
    tp, tu = _time(t, x)
    L.call("gspl_hexplane_fwd", N, lv.n_features, lv.n_levels, _host(lv.resolutions), _host(lv.offsets), _host(box),
           L.ptr(x, torch.float32), L.ptr(tp), tu, L.ptr(table, torch.float32), L.ptr(out), L.stream())
    return out


@_guarded(0)
def hexplane_backward(x: Tensor, t: Union[float, Tensor], table: Tensor, box: np.ndarray, layout: HexPlaneLayout, v_out: Tensor,
                      v_table: Tensor = None, want_x: bool = False, v_x: Tensor = None):
    """The backward launches alone: v_out [N, L * F] -> (v_table, v_x).  `v_table` (the table's shape, contiguous float32) is
    ACCUMULATED into — pass a cleared buffer, or a gradient to add to; None: not computed.  v_x [N, 3] is computed when `want_x`, or
    written into the buffer `v_x` (contiguous float32 [N, 3]) when one is given."""
    lv, N = layout, x.shape[0]
    A.shape("hexplane_backward", "v_out", v_out, (N, lv.n_output_dims))
    if v_table is not None:
        A.buffer("hexplane_backward", "v_table", v_table, lv.n_params, torch.float32, x, contiguous=False)
    v = A.rows16(v_out)
    if v_x is not None:
        A.buffer("hexplane_backward", "v_x", v_x, (N, 3), torch.float32, x, contiguous=False)
    if v_x is None and want_x:
        v_x = torch.empty_like(x)
    if v_table is not None or v_x is not None:
        tp, tu = _time(t, x)
        L.call("gspl_hexplane_bwd", N, lv.n_features, lv.n_levels, _host(lv.resolutions), _host(lv.offsets), _host(box),
               L.ptr(x, torch.float32), L.ptr(tp), tu, L.ptr(table, torch.float32), L.ptr(v), L.ptr(v_table), L.ptr(v_x), L.stream())
    return v_table, v_x


class _HexPlaneFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, table, t, box, layout):
        xc, tc = x.detach().contiguous(), table.detach().contiguous()
        tt = t.detach().reshape(-1).contiguous() if isinstance(t, Tensor) else None
        ctx.save_for_backward(xc, tc, tt)
        ctx.t, ctx.box, ctx.layout, ctx.table_shape = t, box, layout, table.shape
        return hexplane_forward(xc, t if tt is None else tt, tc, box, layout)

    @staticmethod
    def backward(ctx, v_out):
        xc, tc, tt = ctx.saved_tensors
        want_x, want_table = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        v_table = torch.zeros(ctx.table_shape, dtype=torch.float32, device=tc.device) if want_table else None
        v_table, v_x = hexplane_backward(xc, ctx.t if tt is None else tt, tc, ctx.box, ctx.layout, v_out, v_table, want_x)
        return v_x, v_table, None, None, None


def hexplane_encode(x: Tensor, t: Union[float, Tensor], table: Tensor, aabb, layout: HexPlaneLayout) -> Tensor:
    """x [N, 3] float32 on the GPU (any values: outside the box the border texels are used), t ONE python number for the call or a
    float32 tensor [N] / [N, 1] (used as it comes, not normalised), table [total, F] or flat float32 (16-byte aligned) from
    `hexplane_pack`, aabb [2, 3] (tensor or array, aabb[0] the maximum corner as the reference has it) or the [6] array of
    `hexplane_box`, layout from `hexplane_layout` -> [N, L * F] float32,
        out[n, l * F + f] = product over the six planes of the bilinear sample (align_corners=True, border padding) of channel f.
    The gradient reaches `table` (fp32 atomics: the last bits depend on arrival order) and, only when x.requires_grad, `x`; there is
    none for t.  Rows of the incoming gradient that are entirely zero cost almost nothing in the table's backward.  A non-contiguous
    x is copied; another dtype is refused.  CPU tensors raise RuntimeError: there is no fallback."""
    if not isinstance(layout, HexPlaneLayout):
        raise TypeError("hexplane_encode: layout must come from ops.hexplane_layout")
    who = "hexplane_encode"      # (a per-frame call: each test stands here, and `_args` is entered only to refuse)
    if not isinstance(x, Tensor) or not isinstance(table, Tensor):
        A.tensor(who, "x", x)
        A.tensor(who, "table", table)
    if not x.is_cuda or not table.is_cuda or table.device != x.device:
        A.on_gpu(who, "x", x)
        A.on_gpu(who, "table", table, x, "x")
    if x.dtype != torch.float32 or table.dtype != torch.float32:
        A.dtype(who, "x", x, torch.float32)
        A.dtype(who, "table", table, torch.float32)
    if x.dim() != 2 or x.shape[1] != 3:
        A.shape(who, "x", x, ("N", 3))
    if tuple(table.shape) not in ((layout.n_params,), (layout.total, layout.n_features)):
        raise ValueError(f"hexplane_encode: table must be [{layout.total}, {layout.n_features}] or flat [{layout.n_params}], got {tuple(table.shape)}")
    if x.shape[0] >= 2 ** 31:
        raise NotImplementedError(f"hexplane_encode: N = {x.shape[0]} points; fewer than 2^31 are built")
    if table.data_ptr() % 16:
        A.aligned16(who, "table", table)
    return _HexPlaneFn.apply(x, table, t, hexplane_box(aabb), layout)

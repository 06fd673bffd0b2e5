"""Multiresolution hash-grid / dense-grid encoding: the ONE primitive of `tinycudann` that the SWAG route needs
(internal/models/swag_model.py:75-78; include/gspl_hip.h section 20, csrc/hashgrid.hip).

  hashgrid_levels(n_input_dims, n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense=False)
      -> HashGridLevels: the level table (scales, resolutions, sizes, offsets, hashed flags, total), pure numpy, usable on the CPU.
  hashgrid_encode(x, table, levels) -> [N, n_levels * n_features_per_level]
      linear interpolation of the table's rows at x; differentiable in `table`, and in `x` when x requires a gradient.
  hashgrid_table(levels, seed=1337, device=None) -> a new flat table, uniform in [-1e-4, 1e-4] from a seeded generator.
  hashgrid_forward / hashgrid_backward: the launches alone, outside autograd, into the caller's buffers.

GPU only, float32; no fallback.  Parity with tiny-cuda-nn's own build is UNPINNED (there is no ROCm build of it): these are its
published rules, checked against the fp64 oracle tests/hashgrid_oracle.py."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch
from torch import Tensor

from .. import _lib as L
from . import _args as A
from ._args import host_ptr as _host
from ._common import _guarded

MAX_LEVELS = 32
FEATURES = (1, 2, 4, 8)
_MAX_LEVEL_ROWS = (2 ** 32 - 1) // 2


@dataclass(frozen=True)
class HashGridLevels:
    """The level table of a grid encoding.  scales [L] float32, resolutions / sizes [L] uint32, offsets [L + 1] uint32 (offsets[l] is
    the first row of level l, offsets[L] == total), hashed [L] bool; the table has `total` rows of `n_features_per_level` floats."""
    n_input_dims: int
    n_levels: int
    n_features_per_level: int
    scales: np.ndarray
    resolutions: np.ndarray
    sizes: np.ndarray
    offsets: np.ndarray
    hashed: np.ndarray
    total: int

    @property
    def n_output_dims(self) -> int:
        return self.n_levels * self.n_features_per_level

    @property
    def n_params(self) -> int:
        return self.total * self.n_features_per_level


def hashgrid_levels(n_input_dims: int, n_levels: int, n_features_per_level: int, log2_hashmap_size: int, base_resolution: int,
                    per_level_scale: float, dense: bool = False) -> HashGridLevels:
    """The level table, computed on the host in double and rounded once:
        scale_l = float32(exp2(l * log2(per_level_scale)) * base_resolution - 1);   res_l = ceil(scale_l) + 1
        size_l  = min(res_l ** D, (2**32 - 1) // 2) rounded up to a multiple of 8, and unless `dense` capped at 2 ** log2_hashmap_size
    A level is hashed iff res_l ** D > size_l; its offset is the running sum of the sizes.  `dense=True` (otype DenseGrid) ignores
    log2_hashmap_size; a dense level that would not fit its rows is refused."""
    D, n_levels, F = int(n_input_dims), int(n_levels), int(n_features_per_level)
    if D not in (2, 3):
        raise NotImplementedError(f"hashgrid_levels: n_input_dims 2 and 3 are built, got {n_input_dims}")
    if not 1 <= n_levels <= MAX_LEVELS:
        raise ValueError(f"hashgrid_levels: n_levels must be 1 .. {MAX_LEVELS}, got {n_levels}")
    if F not in FEATURES:
        raise NotImplementedError(f"hashgrid_levels: n_features_per_level must be one of {FEATURES}, got {n_features_per_level}")
    if int(base_resolution) < 1:
        raise ValueError(f"hashgrid_levels: base_resolution must be at least 1, got {base_resolution}")
    if not float(per_level_scale) > 0 or not math.isfinite(float(per_level_scale)):
        raise ValueError(f"hashgrid_levels: per_level_scale must be positive and finite, got {per_level_scale}")
    if not dense and not 0 <= int(log2_hashmap_size) <= 31:
        raise ValueError(f"hashgrid_levels: log2_hashmap_size must be 0 .. 31, got {log2_hashmap_size}")
    log2_scale = math.log2(float(per_level_scale))
    scales, resolutions, sizes, hashed = [], [], [], []
    for level in range(n_levels):
        scale = np.float32(2.0 ** (level * log2_scale) * float(base_resolution) - 1.0)
        if not scale < 2.0 ** 30:
            raise ValueError(f"hashgrid_levels: level {level} has a resolution beyond 2^30 (per_level_scale {per_level_scale})")
        res = int(math.ceil(float(scale))) + 1
        cells = res ** D
        size = -(-min(cells, _MAX_LEVEL_ROWS) // 8) * 8
        if not dense:
            size = min(size, 2 ** int(log2_hashmap_size))
        elif cells > size:
            raise ValueError(f"hashgrid_levels: dense level {level} of resolution {res} has more than {_MAX_LEVEL_ROWS} cells")
        scales.append(scale)
        resolutions.append(res)
        sizes.append(size)
        hashed.append(cells > size)
    offsets = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
    total = int(offsets[-1])
    if total >= 2 ** 32 or total * F >= 2 ** 40:
        raise ValueError(f"hashgrid_levels: the table would have {total} rows; fewer than 2^32 are built")
    return HashGridLevels(D, n_levels, F, np.asarray(scales, dtype=np.float32), np.asarray(resolutions, dtype=np.uint32),
                          np.asarray(sizes, dtype=np.uint32), offsets.astype(np.uint32), np.asarray(hashed, dtype=bool), total)


def hashgrid_table(levels: HashGridLevels, seed: int = 1337, device=None) -> Tensor:
    """A new flat table [total * F] float32, uniform in [-1e-4, 1e-4] (tiny-cuda-nn's initialisation of a grid), drawn on the CPU from
    a generator seeded with `seed`: the same seed gives the same table on every device."""
    generator = torch.Generator().manual_seed(int(seed))
    table = (torch.rand((levels.n_params,), generator=generator, dtype=torch.float32) * 2 - 1) * 1e-4
    return table if device is None else table.to(device)


@_guarded(0)
def hashgrid_forward(x: Tensor, table: Tensor, levels: HashGridLevels, out: Tensor = None) -> Tensor:
    """The forward launch alone, outside autograd: x [N, D] and table contiguous float32 on the GPU -> out [N, L * F] (written into
    `out` when one is given: contiguous float32 of that shape, 16-byte aligned)."""
    lv, N = levels, x.shape[0]
    if out is None:
        out = torch.empty((N, lv.n_output_dims), dtype=torch.float32, device=x.device)
    else:
        A.buffer("hashgrid_forward", "out", out, (N, lv.n_output_dims), torch.float32, x, contiguous=False)
    L.call("gspl_hashgrid_fwd", N, lv.n_input_dims, lv.n_features_per_level, lv.n_levels, _host(lv.scales), _host(lv.resolutions),
           _host(lv.offsets), L.ptr(x, torch.float32), L.ptr(table, torch.float32), L.ptr(out), L.stream())
    return out


@_guarded(0)
def hashgrid_backward(x: Tensor, table: Tensor, levels: HashGridLevels, v_out: Tensor, v_table: Tensor = None, want_x: bool = False):
    """The backward launches alone: v_out [N, L * F] -> (v_table, v_x).  `v_table` (the table's shape, contiguous float32) is
    ACCUMULATED into — pass a cleared buffer, or a gradient to add to; None: not computed.  v_x [N, D] is computed when `want_x`."""
    lv, N = levels, x.shape[0]
    A.shape("hashgrid_backward", "v_out", v_out, (N, lv.n_output_dims))
    if v_table is not None:
        A.buffer("hashgrid_backward", "v_table", v_table, lv.n_params, torch.float32, x, contiguous=False)
    v = A.rows16(v_out)
    v_x = torch.empty_like(x) if want_x else None
    if v_table is not None or want_x:
        L.call("gspl_hashgrid_bwd", N, lv.n_input_dims, lv.n_features_per_level, lv.n_levels, _host(lv.scales), _host(lv.resolutions),
               _host(lv.offsets), L.ptr(x, torch.float32), L.ptr(table, torch.float32), L.ptr(v), L.ptr(v_table), L.ptr(v_x), L.stream())
    return v_table, v_x


class _HashGridFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, table, levels):
        xc, tc = x.detach().contiguous(), table.detach().contiguous()
        ctx.save_for_backward(xc, tc)
        ctx.levels, ctx.table_shape = levels, table.shape
        return hashgrid_forward(xc, tc, levels)

    @staticmethod
    def backward(ctx, v_out):
        xc, tc = ctx.saved_tensors
        want_x, want_table = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        v_table = torch.zeros(ctx.table_shape, dtype=torch.float32, device=tc.device) if want_table else None
        v_table, v_x = hashgrid_backward(xc, tc, ctx.levels, v_out, v_table, want_x)
        return v_x, v_table, None


def hashgrid_encode(x: Tensor, table: Tensor, levels: HashGridLevels) -> Tensor:
    """x [N, D] float32 on the GPU (any values: cells wrap), table [total, F] or flat [total * F] float32 (16-byte aligned), levels
    from `hashgrid_levels` -> [N, n_levels * F] float32, out[n, l * F + f] = sum over the 2^D corners of weight * table row.
    The gradient reaches `table` (fp32 atomics: the last bits depend on arrival order) and, only when x.requires_grad, `x`.  Rows of
    the incoming gradient that are entirely zero cost almost nothing in the backward.  A non-contiguous x is copied; another dtype
    is refused.  CPU tensors raise RuntimeError: there is no fallback."""
    if not isinstance(levels, HashGridLevels):
        raise TypeError("hashgrid_encode: levels must come from ops.hashgrid_levels")
    who = "hashgrid_encode"      # (a per-frame call: each test stands here, and `_args` is entered only to refuse)
    if not isinstance(x, Tensor) or not isinstance(table, Tensor):
        A.tensor(who, "x", x)
        A.tensor(who, "table", table)
    if not x.is_cuda or not table.is_cuda or table.device != x.device:
        A.on_gpu(who, "x", x)
        A.on_gpu(who, "table", table, x, "x")
    if x.dtype != torch.float32 or table.dtype != torch.float32:
        A.dtype(who, "x", x, torch.float32, error=RuntimeError)
        A.dtype(who, "table", table, torch.float32, error=RuntimeError)
    if x.dim() != 2 or x.shape[1] != levels.n_input_dims:
        A.shape(who, "x", x, ("N", levels.n_input_dims))
    if tuple(table.shape) not in ((levels.n_params,), (levels.total, levels.n_features_per_level)):
        raise ValueError(f"hashgrid_encode: table must be [{levels.total}, {levels.n_features_per_level}] or flat [{levels.n_params}], "
                         f"got {tuple(table.shape)}")
    if x.shape[0] >= 2 ** 31:
        raise ValueError(f"hashgrid_encode: x has {x.shape[0]} rows; fewer than 2^31 are built")
    if table.data_ptr() % 16:
        A.aligned16(who, "table", table)
    return _HashGridFn.apply(x, table, levels)

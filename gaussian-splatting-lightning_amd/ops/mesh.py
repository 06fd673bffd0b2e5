"""TSDF fusion of depth maps and marching tetrahedra: the GPU half of 2DGS mesh extraction (include/gspl_hip.h section 18,
csrc/mesh.hip).

  tsdf_init(M, with_rgb, device) -> (tsdf [M] = 1, weight [M] = 1, color [M, 3] = 0 or None)
      the state the reference starts a fusion from.
  tsdf_table(center, radius, voxel_size, sdf_trunc=None, depth_trunc=None, contract=False, with_rgb=False, lo=None, hi=None, device=...)
      the kernel's 16-float DEVICE table.  Every entry may be a python number or a device tensor: nothing is read back.
  tsdf_fuse(state, table, views, depth, rgb=None, points=None, lattice=None, block=None) -> state
      fuses V views into the state IN PLACE, one launch.  The samples are `points` [M, 3], or the nodes of `lattice` = (n0, n1, n2)
      between the table's lo and hi — optionally only `block` = ((b0, b1, b2), (m0, m1, m2)) of them; the lattice is never materialised.
      A second call continues where the first stopped: the bits of one call over all views.
  marching_tetrahedra(volume, level, origin, step, global_dims=None, block_offset=None) -> (vertices [Nv, 3], faces [T, 3] int64, keys [Nv])
      the iso-surface of volume [X, Y, Z]; vertices shared between triangles are merged through their int64 edge keys
      (`torch.unique` on the device).  origin / step describe the GLOBAL lattice (tensors on the device or sequences of three numbers).
  marching_tetrahedra_soup(...) -> (vertices [3 T, 3], keys [3 T])
      the same before the merge: what the kernels emit, triangle after triangle.

GPU only, float32; no fallback and no autograd (these are `no_grad` ops).  The one host read-back is the triangle total between the
count and the emit launch."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _lib as L
from . import _args as A
from ._common import _guarded

TABLE_FLOATS = L.GSPL_TSDF_TABLE_FLOATS


def _floats(value, n: int, name: str, device) -> Tensor:
    """`value` (a number, a sequence of n numbers or a tensor of n elements) as n float32 on `device`, without a read-back."""
    if isinstance(value, Tensor):
        t = value.detach().to(device=device, dtype=torch.float32).reshape(-1)
    else:
        t = torch.as_tensor(value, dtype=torch.float32).reshape(-1).to(device)
    if t.numel() != n:
        raise ValueError(f"{name} must have {n} element(s), got {t.numel()}")
    return t


def tsdf_init(M: int, with_rgb: bool, device) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """The reference's initial state: tsdf 1, weight 1, colour 0."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("device: the mesh ops run on the GPU only; there is no CPU fallback")
    return (torch.ones(M, dtype=torch.float32, device=device), torch.ones(M, dtype=torch.float32, device=device),
            torch.zeros((M, 3), dtype=torch.float32, device=device) if with_rgb else None)


def tsdf_table(center=(0.0, 0.0, 0.0), radius=1.0, voxel_size=1.0, sdf_trunc=None, depth_trunc=None, contract: bool = False,
               with_rgb: bool = False, lo=None, hi=None, device="cuda") -> Tensor:
    """The DEVICE table of `gspl_tsdf_fuse` (header section 18)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("device: the mesh ops run on the GPU only; there is no CPU fallback")
    zero3 = (0.0, 0.0, 0.0)
    return torch.cat([
        _floats(center, 3, "center", device), _floats(radius, 1, "radius", device), _floats(voxel_size, 1, "voxel_size", device),
        _floats(0.0 if sdf_trunc is None else sdf_trunc, 1, "sdf_trunc", device),
        _floats(0.0 if depth_trunc is None else depth_trunc, 1, "depth_trunc", device),
        _floats(1.0 if contract else 0.0, 1, "contract", device), _floats(1.0 if with_rgb else 0.0, 1, "with_rgb", device),
        _floats(zero3 if lo is None else lo, 3, "lo", device), _floats(zero3 if hi is None else hi, 3, "hi", device),
        _floats(0.0, 1, "pad", device)])


def _ints3(v, name: str) -> Tuple[int, int, int]:
    v = tuple(int(x) for x in v)
    if len(v) != 3:
        raise ValueError(f"{name} must be three integers, got {v}")
    return v


@_guarded(0)
def _fuse(tsdf, weight, color, table, views, depth, rgb, points, n, b, m):
    M, (V, H, W) = tsdf.shape[0], depth.shape
    L.call("gspl_tsdf_fuse", M, L.ptr(points), *n, *b, *m, L.ptr(table), V, H, W, L.ptr(views), L.ptr(depth), L.ptr(rgb),
           L.ptr(tsdf), L.ptr(weight), L.ptr(color), L.stream())


@torch.no_grad()
def tsdf_fuse(state, table: Tensor, views: Tensor, depth: Tensor, rgb: Optional[Tensor] = None, points: Optional[Tensor] = None,
              lattice: Optional[Sequence[int]] = None, block=None):
    """Fuse `depth` [V, H, W] (and `rgb` [V, 3, H, W]) seen through `views` [V, 4, 4] (or [V, 16]) into state = (tsdf, weight, color),
    in place; returns the state.  See the module text and header section 18."""
    tsdf, weight, color = state
    A.gpu_f32("mesh", "tsdf", tsdf, ("M",))
    M = tsdf.shape[0]
    A.gpu_f32("mesh", "weight", weight, (M,), tsdf, "tsdf")
    if color is not None:
        A.gpu_f32("mesh", "color", color, (M, 3), tsdf, "tsdf")
    A.gpu_f32("mesh", "table", table, (TABLE_FLOATS,), tsdf, "tsdf")
    A.gpu_f32("mesh", "depth", depth, None, tsdf, "tsdf")
    if depth.dim() == 4 and depth.shape[1] == 1:
        depth = depth[:, 0]
    if depth.dim() != 3:
        raise ValueError(f"depth must be [V, H, W] (or [V, 1, H, W]), got {list(depth.shape)}")
    V, H, W = depth.shape
    A.gpu_f32("mesh", "views", views, None, tsdf, "tsdf")
    if views.numel() != V * 16 or views.shape[0] != V:
        raise ValueError(f"views must be [{V}, 4, 4] (or [{V}, 16]), got {list(views.shape)}")
    if V > 0 and (H < 1 or W < 1):
        raise ValueError(f"depth maps must not be empty, got {list(depth.shape)}")
    if rgb is not None:
        A.gpu_f32("mesh", "rgb", rgb, (V, 3, H, W), tsdf, "tsdf")
    for t, name in ((tsdf, "tsdf"), (weight, "weight"), (color, "color")):      # (updated in place)
        if t is not None:
            A.contiguous(None, name, t, error=ValueError)
    if points is not None:
        A.gpu_f32("mesh", "points", points, (M, 3), tsdf, "tsdf")
        n = b = m = (0, 0, 0)
    else:
        if lattice is None:
            raise ValueError("tsdf_fuse needs `points` or `lattice`")
        n = _ints3(lattice, "lattice")
        b, m = ((0, 0, 0), n) if block is None else (_ints3(block[0], "block offset"), _ints3(block[1], "block shape"))
        if min(n) < 1 or min(m) < 1 or min(b) < 0 or any(bb + mm > nn for bb, mm, nn in zip(b, m, n)) or m[0] * m[1] * m[2] != M:
            raise ValueError(f"lattice {n} with block {b} + {m} does not describe the state's {M} samples")
    _fuse(tsdf, weight, color, table, views.contiguous(), depth.contiguous(), None if rgb is None else rgb.contiguous(),
          None if points is None else points.contiguous(), n, b, m)
    return state


@_guarded(0)
def _soup(volume, level, grid, G, b):
    X, Y, Z = volume.shape
    dev = volume.device
    empty = (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0,), dtype=torch.int64, device=dev))
    if min(X, Y, Z) < 2:
        return empty
    cells = (X - 1) * (Y - 1) * (Z - 1)
    counts = torch.empty((cells,), dtype=torch.uint8, device=dev)
    L.call("gspl_mtet_count", X, Y, Z, L.ptr(volume), level, L.ptr(counts), L.stream())
    offsets = torch.cumsum(counts, 0, dtype=torch.int32)
    total = int(offsets[-1])                    # the one read-back
    if total == 0:
        return empty
    offsets -= counts                           # exclusive
    del counts
    vertices = torch.empty((3 * total, 3), dtype=torch.float32, device=dev)
    keys = torch.empty((3 * total,), dtype=torch.int64, device=dev)
    L.call("gspl_mtet_emit", X, Y, Z, L.ptr(volume), level, L.ptr(grid), *G, *b, L.ptr(offsets), total, L.ptr(vertices), L.ptr(keys),
           L.stream())
    return vertices, keys


@torch.no_grad()
def marching_tetrahedra_soup(volume: Tensor, level: float, origin, step, global_dims=None, block_offset=None) -> Tuple[Tensor, Tensor]:
    """(vertices [3 T, 3], keys [3 T]) in emission order: cell-major, then tetrahedron, then triangle (header section 18)."""
    A.gpu_f32("mesh", "volume", volume, ("X", "Y", "Z"))
    G = tuple(volume.shape) if global_dims is None else _ints3(global_dims, "global_dims")
    b = (0, 0, 0) if block_offset is None else _ints3(block_offset, "block_offset")
    if min(b) < 0 or any(bb + s > g for bb, s, g in zip(b, volume.shape, G)):
        raise ValueError(f"block {b} + {tuple(volume.shape)} leaves the global lattice {G}")
    grid = torch.cat([_floats(origin, 3, "origin", volume.device), _floats(step, 3, "step", volume.device)])
    return _soup(volume.contiguous(), float(level), grid, G, b)


def index_soup(vertices: Tensor, keys: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """A triangle soup with edge keys -> (vertices [Nv, 3], faces [T, 3] int64, keys [Nv]), keys ascending.  Equal keys hold equal
    positions (header section 18), so any representative serves."""
    unique, inverse = torch.unique(keys, return_inverse=True)
    out = torch.empty((unique.shape[0], 3), dtype=vertices.dtype, device=vertices.device)
    out[inverse] = vertices
    return out, inverse.reshape(-1, 3), unique


@torch.no_grad()
def marching_tetrahedra(volume: Tensor, level: float, origin, step, global_dims=None, block_offset=None) -> Tuple[Tensor, Tensor, Tensor]:
    """The indexed iso-surface of `volume` at `level`: (vertices [Nv, 3], faces [T, 3] int64, keys [Nv])."""
    return index_soup(*marching_tetrahedra_soup(volume, level, origin, step, global_dims, block_offset))

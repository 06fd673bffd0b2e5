"""The per-frame front of the partition-LoD route (internal/renderers/partition_lod_renderer.py:550-625; include/gspl_hip.h
section 26, csrc/lod.hip).

  lod_select(...) -> (distance [P], lod [P] int8, visible [P] u8, dst_start [P + 1] int64, record [2] int64)
      one launch: the distance of every partition's 2-D box from the camera, the level of detail the thresholds give it, the frustum
      test of the visibility filter, the exclusive scan of the chosen segments' lengths and {total rows, changed} for the host.
  lod_gather(...) -> (means, shs, opacities, scales, rotations), the first n rows written
      one launch: the chosen segments of the five flat property arrays, in partition order.

GPU only, float32; no fallback.  Nothing here waits for the device: the caller reads `record` (gspl_amd.lod.LoDSelector does, once
per frame)."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _lib as L
from . import _args as A
from ._common import _guarded

MAX_PARTITIONS = L.GSPL_LOD_MAX_PARTITIONS      # one workgroup loops over them
MAX_LEVELS = L.GSPL_LOD_MAX_LEVELS              # int8 levels; 127 marks "none yet" in the previous frame's array
MAX_COEFFS = L.GSPL_LOD_MAX_COEFFS
PROPERTIES = ("means", "shs", "opacities", "scales", "rotations")


def _widths(K: int):
    return {"means": (3,), "shs": (K, 3), "opacities": (1,), "scales": (3,), "rotations": (4,)}


def _check_all(who: str, checks: Sequence[Tuple[str, object, Optional[tuple], torch.dtype]], anchor: Tensor):
    """(name, tensor, shape, dtype) each, pass by pass in `_args`' order for a machine without a GPU: types, shapes, dtypes, then
    devices and layout.  A shape of None is checked by the caller.  This runs every frame over a dozen tensors, so each test stands
    here and `_args` is entered only to refuse."""
    for name, t, _, _ in checks:
        if not isinstance(t, Tensor):
            A.tensor(who, name, t)
    for name, t, shape, _ in checks:
        if shape is not None and tuple(t.shape) != shape:
            A.shape(who, name, t, shape)
    for name, t, _, dtype in checks:
        if t.dtype != dtype:
            A.dtype(who, name, t, dtype)
    for name, t, _, _ in checks:
        if not t.is_cuda or t.device != anchor.device:
            A.on_gpu(who, name, t, anchor, "the table")
        if not t.is_contiguous():
            A.contiguous(who, name, t)


def _levels(who: str, seg_start, box_min) -> Tuple[int, int]:
    """-> (P, L) from box_min [P, 2] and seg_start [L P + 1]."""
    if not isinstance(seg_start, Tensor) or not isinstance(box_min, Tensor):
        A.tensor(who, "seg_start", seg_start)
        A.tensor(who, "box_min", box_min)
    if box_min.dim() != 2 or box_min.shape[1] != 2 or box_min.shape[0] < 1:
        raise ValueError(f"{who}: box_min must be [P, 2] with P >= 1, got {list(box_min.shape)}")
    P = box_min.shape[0]
    if P > MAX_PARTITIONS:
        raise ValueError(f"{who}: up to {MAX_PARTITIONS} partitions (one workgroup loops over them), got {P}")
    if seg_start.dim() != 1 or seg_start.numel() < P + 1 or (seg_start.numel() - 1) % P:
        raise ValueError(f"{who}: seg_start must be [L * {P} + 1], got {list(seg_start.shape)}")
    levels = (seg_start.numel() - 1) // P
    if levels > MAX_LEVELS:
        raise ValueError(f"{who}: up to {MAX_LEVELS} levels, got {levels}")
    return P, levels


@_guarded(0)
def lod_select(seg_start: Tensor, camera_center: Tensor, transform: Tensor, box_min: Tensor, box_max: Tensor, thresholds: Tensor,
               prev_lod: Tensor, prev_visible: Tensor, boxes3d: Tensor = None, world_to_camera: Tensor = None, Ks: Tensor = None,
               width: int = 0, height: int = 0, visibility_filter: bool = False, distance: Tensor = None, lod: Tensor = None,
               visible: Tensor = None, dst_start: Tensor = None, record: Tensor = None):
    """seg_start [L P + 1] int64, camera_center [3], transform [3, 3], box_min / box_max [P, 2], thresholds [L - 1], prev_lod [P] int8,
    prev_visible [P] uint8 (or bool); with `visibility_filter` also boxes3d [P, 8, 3], world_to_camera [4, 4] (the reference's
    transposed matrix), Ks [3, 3] (or [1, 3, 3]) and the image size.  -> (distance [P], lod [P] int8, visible [P] uint8,
    dst_start [P + 1] int64, record [2] int64 = {total rows, changed}), written into the caller's buffers where given (which may not
    be prev_lod / prev_visible).  Nothing is read back: `record` stays on the device."""
    who = "lod_select"
    P, levels = _levels(who, seg_start, box_min)
    if isinstance(prev_visible, Tensor) and prev_visible.dtype == torch.bool:
        prev_visible = prev_visible.view(torch.uint8)
    if isinstance(Ks, Tensor) and Ks.dim() == 3 and Ks.shape[0] == 1:
        Ks = Ks[0]
    f32 = torch.float32
    checks = [("seg_start", seg_start, (levels * P + 1,), torch.int64), ("camera_center", camera_center, (3,), f32),
              ("transform", transform, (3, 3), f32), ("box_min", box_min, (P, 2), f32), ("box_max", box_max, (P, 2), f32),
              ("thresholds", thresholds, (levels - 1,), f32), ("prev_lod", prev_lod, (P,), torch.int8),
              ("prev_visible", prev_visible, (P,), torch.uint8)]
    if visibility_filter:
        checks += [("boxes3d", boxes3d, (P, 8, 3), f32), ("world_to_camera", world_to_camera, (4, 4), f32), ("Ks", Ks, (3, 3), f32)]
    _check_all(who, checks, seg_start)
    if visibility_filter and (int(width) < 1 or int(height) < 1):
        raise ValueError(f"{who}: the visibility filter needs the image size, got {width} x {height}")
    distance = A.out(who, "distance", distance, (P,), f32, seg_start)
    lod = A.out(who, "lod", lod, (P,), torch.int8, seg_start)
    visible = A.out(who, "visible", visible, (P,), torch.uint8, seg_start)
    dst_start = A.out(who, "dst_start", dst_start, (P + 1,), torch.int64, seg_start)
    record = A.out(who, "record", record, (2,), torch.int64, seg_start)
    if lod.data_ptr() == prev_lod.data_ptr() or visible.data_ptr() == prev_visible.data_ptr():
        raise ValueError(f"{who}: lod / visible may not be the previous frame's arrays")
    on = bool(visibility_filter)
    L.call("gspl_lod_select", P, levels, L.ptr(camera_center), L.ptr(transform), L.ptr(box_min), L.ptr(box_max),
           L.ptr(thresholds) if levels > 1 else None, L.ptr(boxes3d) if on else None, L.ptr(world_to_camera) if on else None,
           L.ptr(Ks) if on else None, int(width), int(height), int(on), L.ptr(seg_start), L.ptr(prev_lod), L.ptr(prev_visible),
           L.ptr(distance), L.ptr(lod), L.ptr(visible), L.ptr(dst_start), L.ptr(record), L.stream())
    return distance, lod, visible, dst_start, record


@_guarded(0)
def lod_gather(seg_start: Tensor, lod: Tensor, dst_start: Tensor, n: int, means: Tensor, shs: Tensor, opacities: Tensor, scales: Tensor,
               rotations: Tensor, out: Sequence[Tensor] = None):
    """The chosen segments of the flat table (means [R, 3], shs [R, K, 3], opacities [R, 1], scales [R, 3], rotations [R, 4];
    seg_start [L P + 1] int64 over its rows) -> five arrays whose first `n` rows are the rows of segment (lod[p], p) for p = 0 .. P - 1
    at rows dst_start[p] .. dst_start[p + 1].  `n` is the total `lod_select` left in its record (the host has read it).  `out`: five
    buffers of at least n rows each, in the table's order; rows from n on are left as they are.  Bit-exact copies, one launch."""
    who = "lod_gather"
    for name, t in (("seg_start", seg_start), ("lod", lod), ("dst_start", dst_start), ("means", means), ("shs", shs)):
        A.tensor(who, name, t)
    if lod.dim() != 1 or lod.numel() < 1:
        raise ValueError(f"{who}: lod must be [P], got {list(lod.shape)}")
    P = lod.numel()
    if P > MAX_PARTITIONS:
        raise ValueError(f"{who}: up to {MAX_PARTITIONS} partitions, got {P}")
    if seg_start.dim() != 1 or seg_start.numel() < P + 1 or (seg_start.numel() - 1) % P:
        raise ValueError(f"{who}: seg_start must be [L * {P} + 1], got {list(seg_start.shape)}")
    levels = (seg_start.numel() - 1) // P
    if levels > MAX_LEVELS:
        raise ValueError(f"{who}: up to {MAX_LEVELS} levels, got {levels}")
    if means.dim() != 2 or shs.dim() != 3:
        raise ValueError(f"{who}: means must be [R, 3] and shs [R, K, 3], got {list(means.shape)} and {list(shs.shape)}")
    R, K = means.shape[0], shs.shape[1]
    if not 1 <= K <= MAX_COEFFS:
        raise ValueError(f"{who}: shs must hold 1 .. {MAX_COEFFS} coefficients per row, got {K}")
    n = int(n)
    if not 0 <= n <= R:
        raise ValueError(f"{who}: n must be 0 .. {R} (the table's rows), got {n}")
    f32 = torch.float32
    table = dict(zip(PROPERTIES, (means, shs, opacities, scales, rotations)))
    checks = [("seg_start", seg_start, (levels * P + 1,), torch.int64), ("lod", lod, (P,), torch.int8), ("dst_start", dst_start, (P + 1,), torch.int64)]
    checks += [(name, table[name], (R,) + w, f32) for name, w in _widths(K).items()]
    if out is not None:
        if len(out) != 5:
            raise ValueError(f"{who}: out must hold five buffers ({', '.join(PROPERTIES)})")
        for (name, w), t in zip(_widths(K).items(), out):
            A.tensor(who, f"out {name}", t)
            if t.dim() != 1 + len(w) or tuple(t.shape[1:]) != w or t.shape[0] < n:
                raise ValueError(f"{who}: out {name} must be [>= {n}, {', '.join(map(str, w))}], got {list(t.shape)}")
            checks.append((f"out {name}", t, None, f32))
    _check_all(who, checks, seg_start)
    if out is None:
        out = [torch.empty((n,) + w, dtype=f32, device=seg_start.device) for w in _widths(K).values()]
    L.call("gspl_lod_gather", P, levels, K, R, n, L.ptr(seg_start), L.ptr(lod), L.ptr(dst_start), *[L.ptr(table[k]) for k in PROPERTIES],
           *[L.ptr(t) for t in out], L.stream())
    return tuple(out)

"""The partition-LoD route's state between frames (internal/renderers/partition_lod_renderer.py): a city-scale scene cut into
partitions, each trained at several levels of detail, shown by picking one level per partition for every frame.

  LoDTable      every (level, partition) model packed ONCE into five flat device arrays + `seg_start`; owns the destination buffers
                the gather writes (grown geometrically, never shrunk) and hands out [:n] views of them.
  LoDSelector   the device state (`lod`, `visible`, thresholds) and the per-frame sequence: `ops.lod_select`, ONE read of its 16-byte
                record, `ops.lod_gather` only when the selection changed and `freeze` is off.
  GatheredModel the frozen, pre-activated model the inner renderer reads: the table's current views.

The reference keeps a list of models per level and, when the selection changes, walks the partitions in Python with one `.item()`
each and concatenates five lists of tensors; it compares the selection with the previous frame's through two `torch.all(torch.eq())`
host waits on every frame.

Not built (NotImplementedError where asked for): `partition_size` re-division, per-partition appearance models (`update_shs_dc`),
models that carry a Mip-Splatting 3D filter."""
from __future__ import annotations

from typing import Dict, List, Sequence

import torch
from torch import Tensor

from . import ops
from .ops.lod import PROPERTIES, MAX_LEVELS, MAX_PARTITIONS, MAX_COEFFS

NO_LEVEL = 127      # what the reference fills `partition_lods` with before the first frame


def _model_properties(entry, where: str) -> Dict[str, Tensor]:
    """A property dict, or a pre-activated model (`properties` with means / shs / opacities / scales / rotations), as the five arrays."""
    if hasattr(entry, "compute_3d_filter") or (hasattr(entry, "properties") and any("filter_3d" in k for k in entry.properties)):
        raise NotImplementedError(f"LoDTable: {where} carries a Mip-Splatting 3D filter; applying it to the scales and opacities "
                                  f"(MipSplattingUtils.apply_3d_filter_on_scales) is not built")
    if hasattr(entry, "shs_dc_backup") or (not isinstance(entry, dict) and hasattr(entry, "get_appearance_features")):
        raise NotImplementedError(f"LoDTable: {where} carries appearance features; per-partition appearance models "
                                  f"(`update_shs_dc`) are not built")
    props = entry if isinstance(entry, dict) else getattr(entry, "properties", None)
    if props is None:
        raise TypeError(f"LoDTable: {where} must be a dict of properties or a model with `properties`, got {type(entry).__name__}")
    if not isinstance(entry, dict) and not getattr(entry, "is_pre_activated", False):
        raise ValueError(f"LoDTable: {where} is not pre-activated (`pre_activate_all_properties()`): the table stores activated values")
    props = dict(props)
    if "shs" not in props and "shs_dc" in props and "shs_rest" in props:
        props["shs"] = torch.cat((props["shs_dc"], props["shs_rest"]), dim=1)
    missing = [k for k in PROPERTIES if k not in props]
    if missing:
        raise ValueError(f"LoDTable: {where} lacks {missing} (has {sorted(props)})")
    return {k: props[k].detach() for k in PROPERTIES}


class LoDTable:
    """levels: [L][P] property dicts or pre-activated models, finest level first; every level holds the same P partitions.
    Packed once: means [R, 3], shs [R, K, 3], opacities [R, 1], scales [R, 3], rotations [R, 4] on `device`, segment (l, p) at rows
    seg_start[l P + p] .. seg_start[l P + p + 1].  `drop_shs_rest` keeps the DC coefficient only (K = 1), as the reference's option."""

    def __init__(self, levels: Sequence[Sequence], device="cuda", drop_shs_rest: bool = False):
        if len(levels) < 1 or len(levels[0]) < 1:
            raise ValueError("LoDTable: at least one level of at least one partition")
        self.n_levels, self.n_partitions = len(levels), len(levels[0])
        if self.n_levels > MAX_LEVELS or self.n_partitions > MAX_PARTITIONS:
            raise ValueError(f"LoDTable: up to {MAX_LEVELS} levels of {MAX_PARTITIONS} partitions, got {self.n_levels} x {self.n_partitions}")
        if any(len(level) != self.n_partitions for level in levels):
            raise ValueError(f"LoDTable: every level must hold {self.n_partitions} partitions, got {[len(level) for level in levels]}")
        segments = [_model_properties(entry, f"level {l} partition {p}") for l, level in enumerate(levels) for p, entry in enumerate(level)]
        K = 1 if drop_shs_rest else segments[0]["shs"].shape[1]
        widths = {"means": (3,), "shs": (K, 3), "opacities": (1,), "scales": (3,), "rotations": (4,)}
        lengths = []
        for i, seg in enumerate(segments):
            n = seg["means"].shape[0]
            if drop_shs_rest:
                seg["shs"] = seg["shs"][:, :1]
            for k, w in widths.items():
                if tuple(seg[k].shape) != (n,) + w:
                    raise ValueError(f"LoDTable: level {i // self.n_partitions} partition {i % self.n_partitions}: {k} must be "
                                     f"{[n, *w]}, got {list(seg[k].shape)}")
            lengths.append(n)
        if not 1 <= K <= MAX_COEFFS:
            raise ValueError(f"LoDTable: 1 .. {MAX_COEFFS} SH coefficients per Gaussian, got {K}")
        self.device = torch.device(device)
        self.n_coeffs, self.sh_degree = K, int(round(K ** 0.5)) - 1
        self.segment_lengths = lengths
        starts = [0]
        for n in lengths:
            starts.append(starts[-1] + n)
        self.n_rows = starts[-1]
        self.seg_start = torch.tensor(starts, dtype=torch.int64).to(self.device)
        self.arrays = {k: torch.cat([seg[k].to(dtype=torch.float32) for seg in segments], dim=0).contiguous().to(self.device) for k in PROPERTIES}
        self._widths = widths
        self._buffers: Dict[str, Tensor] = {}
        self.capacity = 0
        self.n_current = 0

    def segment_length(self, level: int, partition: int) -> int:
        return self.segment_lengths[level * self.n_partitions + partition]

    def reserve(self, n: int) -> List[Tensor]:
        """The five destination buffers with room for n rows: grown to max(n, 2 x capacity) when too small, never shrunk.  (A grown
        buffer's old rows are not kept: the gather that asked for it writes every row it hands out.)"""
        if n > self.capacity or not self._buffers:
            self.capacity = min(max(n, 2 * self.capacity, 1), max(self.n_rows, 1))
            self._buffers = {k: torch.empty((self.capacity,) + w, dtype=torch.float32, device=self.device) for k, w in self._widths.items()}
        return [self._buffers[k] for k in PROPERTIES]

    def views(self, n: int = None) -> Dict[str, Tensor]:
        n = self.n_current if n is None else n
        if not self._buffers:
            self.reserve(0)
        return {k: self._buffers[k][:n] for k in PROPERTIES}


class LoDSelector:
    """boxes: `min` / `max` [P, 2] (the partitions' 2-D boxes in the oriented frame), optionally `corners` [P, 8, 3] (world space,
    the reference's `partition_full_3d_bounding_box`, needed by the visibility filter).  thresholds [L - 1], rising."""

    def __init__(self, table: LoDTable, box_min: Tensor, box_max: Tensor, thresholds, orientation_transform: Tensor = None,
                 corners: Tensor = None):
        dev, P, levels = table.device, table.n_partitions, table.n_levels
        f32 = dict(dtype=torch.float32, device=dev)
        self.table = table
        self.box_min, self.box_max = box_min.detach().to(**f32).contiguous(), box_max.detach().to(**f32).contiguous()
        if tuple(self.box_min.shape) != (P, 2) or tuple(self.box_max.shape) != (P, 2):
            raise ValueError(f"LoDSelector: the boxes must be [{P}, 2], got {list(box_min.shape)} and {list(box_max.shape)}")
        self.transform = (torch.eye(3) if orientation_transform is None else orientation_transform.detach()).to(**f32).contiguous()
        self.corners = None if corners is None else corners.detach().to(**f32).contiguous()
        if self.corners is not None and tuple(self.corners.shape) != (P, 8, 3):
            raise ValueError(f"LoDSelector: corners must be [{P}, 8, 3], got {list(corners.shape)}")
        self.thresholds = torch.zeros(levels - 1, **f32)
        self.update_thresholds(thresholds)
        # two sets of (lod, visible, dst_start): the stored selection and the one a frame writes; they swap, together, when a frame's
        # selection is taken, so that the three public arrays always describe ONE selection, the gathered one.  `distance` is the
        # latest frame's, taken or not (the reference's `partition_distances`).
        self.lod = torch.full((P,), NO_LEVEL, dtype=torch.int8, device=dev)
        self.visible = torch.ones(P, dtype=torch.uint8, device=dev)
        self.dst_start = torch.zeros(P + 1, dtype=torch.int64, device=dev)
        self._lod_next, self._visible_next, self._dst_start_next = torch.empty_like(self.lod), torch.empty_like(self.visible), torch.empty_like(self.dst_start)
        self.distance = torch.zeros(P, **f32)
        self.record = torch.zeros(2, dtype=torch.int64, device=dev)
        self.n_selects = self.n_gathers = 0
        self.n_gaussians = 0

    def update_thresholds(self, values):
        """New distance thresholds (the viewer's "Max Distance" numbers): written into the device array in place (a small host-to-device
        copy)."""
        values = torch.as_tensor(values, dtype=torch.float32).reshape(-1)
        if values.numel() != self.thresholds.numel():
            raise ValueError(f"LoDSelector: {self.thresholds.numel()} thresholds (levels - 1), got {values.numel()}")
        self.thresholds.copy_(values)

    def select(self, camera_center: Tensor, world_to_camera: Tensor = None, Ks: Tensor = None, width: int = 0, height: int = 0,
               visibility_filter: bool = False, freeze: bool = False) -> bool:
        """One frame: select, read the record (the frame's only host wait), gather when the selection changed and `freeze` is off.
        -> whether the gathered set changed.  `table.views()` are the current arrays afterwards.  The camera's tensors are taken in
        any layout: the reference's `world_to_camera` is a transposed VIEW (internal/cameras/cameras.py stores
        `torch.transpose(...)` and slices it), which is copied to a contiguous matrix here, a launch without a wait."""
        if visibility_filter and self.corners is None:
            raise ValueError("LoDSelector: the visibility filter needs the partitions' 3-D corners")
        t = self.table
        dense = lambda m: None if m is None else m.detach().to(dtype=torch.float32).contiguous()
        ops.lod_select(t.seg_start, dense(camera_center.reshape(3)), self.transform, self.box_min, self.box_max, self.thresholds,
                       self.lod, self.visible, self.corners, dense(world_to_camera), dense(Ks), width, height, visibility_filter,
                       distance=self.distance, lod=self._lod_next, visible=self._visible_next, dst_start=self._dst_start_next, record=self.record)
        self.n_selects += 1
        total, changed = self.record.tolist()
        if freeze or not changed:
            return False
        self.lod, self._lod_next = self._lod_next, self.lod
        self.visible, self._visible_next = self._visible_next, self.visible
        self.dst_start, self._dst_start_next = self._dst_start_next, self.dst_start
        ops.lod_gather(t.seg_start, self.lod, self.dst_start, total, *[t.arrays[k] for k in PROPERTIES], out=t.reserve(total))
        self.n_gathers += 1
        t.n_current = self.n_gaussians = total
        return True


class GatheredModel:
    """What the gsplat-v1 plugin reads of a frozen, pre-activated vanilla model (internal/models/vanilla_gaussian.py after
    `pre_activate_all_properties` and `freeze`), over the table's current views."""
    is_pre_activated = True

    def __init__(self, table: LoDTable):
        self.table = table
        self.active_sh_degree = self.max_sh_degree = table.sh_degree
        self.properties = table.views(0)

    n_gaussians = property(lambda self: self.properties["means"].shape[0])
    get_xyz = property(lambda self: self.properties["means"])
    get_features = property(lambda self: self.properties["shs"])
    get_scaling = property(lambda self: self.properties["scales"])
    get_rotation = property(lambda self: self.properties["rotations"])
    get_opacity = property(lambda self: self.properties["opacities"])

    def get_means(self): return self.properties["means"]
    def get_shs(self): return self.properties["shs"]
    def get_scales(self): return self.properties["scales"]
    def get_rotations(self): return self.properties["rotations"]
    def get_opacities(self): return self.properties["opacities"]

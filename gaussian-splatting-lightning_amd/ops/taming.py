"""The scoring arithmetic of the Taming-3DGS density controller (internal/density_controllers/taming_3dgs_density_controller.py:
`Taming3DGSUtils.normalize` :455-465, the aggregate of `compute_gaussian_score` :536-553, `get_edges` :367-373 and the min-max
normalisation of `on_train_start` :138; include/gspl_hip.h section 27, csrc/taming.hip).

  positive_medians(rows) -> (counts [R] int32, medians [R] f32): per row the number of entries > 0 (NaN is none) and `torch.median` of
      them, the lower of the two middle ones; NaN where there is none.  An exact radix select, all rows in one set of passes.
  taming_score_accumulate_(importance, rows, coeffs, counts, medians, w, visible, n_first=5) -> importance, updated in place:
      importance += w * (sum_r coeffs[r] * rows[r] / medians[r] over the valid entries) * visible, in the reference's association.
  find_edges(image) -> [H, W] f32: PIL's `convert('L')` and `FIND_EDGES` on the image as `ToPILImage` quantises it, / 255, min-max
      normalised.  A constant EDGE image (a black image, a constant one without an interior pixel) gives NaN throughout (0 / 0), as the
      reference does; `normalize` later drops NaN.

Rows are float32 or int32 (`radii`), 1-D, of one length; int32 entries stand for float(x).  An entry is valid when its float32 bit
pattern has the sign clear, is non-zero and is at most +inf's: the flush mode of subnormals does not enter.  No row is written (the
reference's in-place NaN -> 0 is not observable by its caller).  Nothing here waits for the device: counts and medians stay on it.

Where they run: tensors on the GPU go to the HIP kernels, and a missing library is an error, never a torch fallback.  Tensors on the CPU
take the plain-torch restatement below (the same rules, float32, in the same association): it is what the CPU tests and the golden
files exercise, and it is chosen by the inputs' device alone.  Mixed devices are refused."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _lib as L
from . import _args as A
from ._common import _guarded

MAX_ROWS = L.GSPL_TAMING_MAX_ROWS
MAX_N = 2 ** 31 - 1
_INF_BITS = 0x7f800000


def _rows(who: str, rows) -> Tuple[Sequence[Tensor], int]:
    if isinstance(rows, Tensor) or not isinstance(rows, (list, tuple)):
        raise TypeError(f"{who}: rows must be a list or tuple of 1-D tensors, got {type(rows).__name__}")
    if not 1 <= len(rows) <= MAX_ROWS:
        raise ValueError(f"{who}: 1 .. {MAX_ROWS} rows, got {len(rows)}")
    for i, t in enumerate(rows):
        A.tensor(who, f"rows[{i}]", t)
    N = rows[0].numel()
    for i, t in enumerate(rows):
        A.shape(who, f"rows[{i}]", t, (N,))
    if not 1 <= N <= MAX_N:
        raise ValueError(f"{who}: rows must hold 1 .. 2^31 - 1 entries, got {N}")
    for i, t in enumerate(rows):
        A.dtype(who, f"rows[{i}]", t, torch.float32, torch.int32)
    for i, t in enumerate(rows):
        if t.device != rows[0].device:
            raise RuntimeError(f"{who}: rows[{i}] is on {t.device}, rows[0] on {rows[0].device}")
    return [t.detach() for t in rows], N


def _gpu_rows(who: str, rows: Sequence[Tensor]):
    """-> (the contiguous rows, kept alive by the caller; the host table of their addresses; the host array of int32 flags)"""
    rows = [A.contiguous(who, f"rows[{i}]", t) for i, t in enumerate(rows)]
    table = (ctypes.c_void_p * len(rows))(*[t.data_ptr() for t in rows])
    flags = (ctypes.c_int32 * len(rows))(*[1 if t.dtype == torch.int32 else 0 for t in rows])
    return rows, table, flags


def valid_entries(row: Tensor) -> Tuple[Tensor, Tensor]:
    """(the row as float32, the mask of its valid entries): > 0 and not NaN, read off the bit pattern."""
    v = row.to(torch.float32)
    bits = v.contiguous().view(torch.int32)
    return v, (bits > 0) & (bits <= _INF_BITS)


def _positive_medians_cpu(rows: Sequence[Tensor]) -> Tuple[Tensor, Tensor]:
    counts = torch.zeros((len(rows),), dtype=torch.int32)
    medians = torch.full((len(rows),), float("nan"), dtype=torch.float32)
    for r, row in enumerate(rows):
        v, ok = valid_entries(row)
        counts[r] = ok.sum()
        if counts[r] > 0:
            medians[r] = torch.median(v[ok])
    return counts, medians


@_guarded(0)
def _positive_medians_gpu(anchor: Tensor, rows: Sequence[Tensor], N: int, counts, medians) -> Tuple[Tensor, Tensor]:
    who = "positive_medians"
    R = len(rows)
    rows, table, flags = _gpu_rows(who, rows)
    counts = A.out(who, "counts", counts, (R,), torch.int32, anchor)
    medians = A.out(who, "medians", medians, (R,), torch.float32, anchor)
    ws_bytes = L.lib().gspl_positive_medians_workspace_bytes(R)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=anchor.device)
    L.call("gspl_positive_medians", R, N, table, flags, L.ptr(counts), L.ptr(medians), L.ptr(ws), ws_bytes, L.stream())
    return counts, medians


def positive_medians(rows: Sequence[Tensor], counts: Optional[Tensor] = None, medians: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """rows: 1 .. 16 tensors [N], float32 or int32, on one device -> (counts [R] int32, medians [R] float32) on that device, written into
    the caller's buffers where given.  medians[r] is the valid entry of rank (counts[r] - 1) // 2 in ascending order, bit for bit
    `torch.median(v[v > 0])`; NaN when counts[r] == 0.  Exact and identical between runs; the rows are not modified."""
    who = "positive_medians"
    rows, N = _rows(who, rows)
    if rows[0].is_cuda:
        return _positive_medians_gpu(rows[0], rows, N, counts, medians)
    c, m = _positive_medians_cpu(rows)
    if counts is not None:
        c = A.buffer(who, "counts", counts, (len(rows),), torch.int32, rows[0]).copy_(c)
    if medians is not None:
        m = A.buffer(who, "medians", medians, (len(rows),), torch.float32, rows[0]).copy_(m)
    return c, m


def _score_cpu(importance: Tensor, rows, coeffs, counts, medians, w, visible, n_first: int) -> Tensor:
    groups = []
    for lo, hi in ((0, n_first), (n_first, len(rows))):
        total = None
        for r in range(lo, hi):
            v, ok = valid_entries(rows[r])
            term = torch.zeros_like(v)
            if int(counts[r]) > 0:
                term[ok] = torch.tensor(coeffs[r], dtype=torch.float32) * (v[ok] / medians[r])
            total = term if total is None else total + term
        groups.append(total)
    first, rest = groups
    s = first if rest is None else rest + first
    importance += (w.reshape(()) * s) * visible.to(torch.float32)
    return importance


@_guarded(0)
def _score_gpu(importance: Tensor, rows, N: int, coeffs, counts, medians, w, visible, n_first: int) -> Tensor:
    who = "taming_score_accumulate_"
    rows, table, flags = _gpu_rows(who, rows)
    c = (ctypes.c_float * len(rows))(*coeffs)
    L.call("gspl_taming_score_accumulate", len(rows), n_first, N, table, flags, c, L.ptr(counts), L.ptr(medians), L.ptr(w), L.ptr(visible),
           L.ptr(importance), L.stream())
    return importance


def taming_score_accumulate_(importance: Tensor, rows: Sequence[Tensor], coeffs: Sequence[float], counts: Tensor, medians: Tensor,
                             w: Tensor, visible: Tensor, n_first: int = 5) -> Tensor:
    """importance [N] float32, updated in place and returned; rows as for `positive_medians` (whose `counts` and `medians` of these
    rows go in); coeffs: R Python floats, the `ScoreCoefficients` multipliers; w: one float32 element on the device (the view's
    `view_importance * photometric_loss`, never read by the host); visible [N] bool or uint8.  The first `n_first` rows are the
    reference's per-Gaussian terms, the others its per-pixel terms:

        importance[g] += (w * ((t_nf + ... + t_{R-1}) + (t_0 + ... + t_{nf-1}))) * visible[g],   t_r = coeffs[r] * (rows[r][g] / medians[r])

    each group added left to right, a term being 0 where the entry is not valid or the row has no valid entry."""
    who = "taming_score_accumulate_"
    rows, N = _rows(who, rows)
    R = len(rows)
    A.tensor(who, "importance", importance)
    for name, t in (("counts", counts), ("medians", medians), ("w", w), ("visible", visible)):
        A.tensor(who, name, t)
    if isinstance(coeffs, Tensor) or len(coeffs) != R:
        raise ValueError(f"{who}: coeffs must be {R} Python floats (one per row)")
    coeffs = [float(c) for c in coeffs]
    if not 1 <= int(n_first) <= R:
        raise ValueError(f"{who}: n_first must be 1 .. {R}, got {n_first}")
    A.shape(who, "importance", importance, (N,))
    A.shape(who, "counts", counts, (R,))
    A.shape(who, "medians", medians, (R,))
    A.numel(who, "w", w, 1)
    A.shape(who, "visible", visible, (N,))
    A.dtype(who, "importance", importance, torch.float32)
    A.dtype(who, "counts", counts, torch.int32)
    A.dtype(who, "medians", medians, torch.float32)
    A.dtype(who, "w", w, torch.float32)
    A.dtype(who, "visible", visible, torch.bool, torch.uint8)
    for name, t in (("importance", importance), ("counts", counts), ("medians", medians), ("w", w), ("visible", visible)):
        if t.device != rows[0].device:
            raise RuntimeError(f"{who}: {name} is on {t.device}, the rows on {rows[0].device}")
    if importance.requires_grad:
        raise RuntimeError(f"{who}: importance is updated in place and may not require a gradient")
    if not rows[0].is_cuda:
        return _score_cpu(importance, rows, coeffs, counts, medians, w.detach(), visible, int(n_first))
    A.contiguous(who, "importance", importance)
    visible = A.contiguous(who, "visible", visible.detach())
    if visible.dtype == torch.bool:
        visible = visible.view(torch.uint8)
    return _score_gpu(importance, rows, N, coeffs, A.contiguous(who, "counts", counts), A.contiguous(who, "medians", medians),
                      w.detach().reshape(1), visible, int(n_first))


def _grey_bytes(image: Tensor) -> Tensor:
    """[3, H, W] uint8 or float32 -> [H, W] int32, PIL's L conversion of the image as ToPILImage quantises it."""
    if image.dtype == torch.float32:
        image = (image * 255.).nan_to_num(0.).clamp(0., 255.).to(torch.uint8)       # `pic.mul(255).byte()`: truncation
    c = image.to(torch.int32)
    return (c[0] * 19595 + c[1] * 38470 + c[2] * 7471 + 0x8000) >> 16


def edge_bytes(image: Tensor) -> Tensor:
    """[3, H, W] -> [H, W] int32 in 0 .. 255: PIL's `convert('L').filter(ImageFilter.FIND_EDGES)` (the 3x3 kernel of -1 with centre 8,
    clipped; the one-pixel border is the grey image unfiltered).  Plain torch, any device."""
    g = _grey_bytes(image)
    e = g.clone()
    H, W = g.shape
    if H >= 3 and W >= 3:
        around = sum(g[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
        e[1:-1, 1:-1] = (8 * g[1:-1, 1:-1] - around).clamp(0, 255)
    return e


def _find_edges_cpu(image: Tensor) -> Tensor:
    x = edge_bytes(image).to(torch.float32) / 255.
    return (x - torch.min(x)) / (torch.max(x) - torch.min(x))


@_guarded(0)
def _find_edges_gpu(image: Tensor, out: Optional[Tensor]) -> Tensor:
    who = "find_edges"
    _, H, W = image.shape
    image = A.contiguous(who, "image", image)
    out = A.out(who, "out", out, (H, W), torch.float32, image)
    n_partial = L.lib().gspl_find_edges_partials(H, W)
    if n_partial == 0:
        raise ValueError(f"{who}: H W must be at most 2^31 - 1, got {H} x {W}")
    partial = torch.empty((n_partial, 2), dtype=torch.int32, device=image.device)
    L.call("gspl_find_edges", H, W, L.ptr(image), int(image.dtype == torch.float32), L.ptr(out), L.ptr(partial), n_partial, L.stream())
    return out


def find_edges(image: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """image [3, H, W], uint8 or float32 in [0, 1] -> [H, W] float32: the reference's `get_edges(image).squeeze(0)` min-max normalised
    (`on_train_start`).  Floats are quantised as `ToPILImage` does, x * 255 truncated to a byte; for uint8 the reference's / 255 and
    * 255 round trip is the identity, so the bytes are read directly.  Where the edge image is constant (a black image, a constant
    one without an interior pixel) the result is NaN throughout (0 / 0)."""
    who = "find_edges"
    A.tensor(who, "image", image)
    A.shape(who, "image", image, (3, "H", "W"))
    if image.shape[1] < 1 or image.shape[2] < 1:
        raise ValueError(f"{who}: image must be [3, H, W] with H, W >= 1, got {list(image.shape)}")
    A.dtype(who, "image", image, torch.uint8, torch.float32)
    image = image.detach()
    if image.is_cuda:
        return _find_edges_gpu(image, out)
    e = _find_edges_cpu(image)
    return e if out is None else A.buffer(who, "out", out, tuple(e.shape), torch.float32, image).copy_(e)

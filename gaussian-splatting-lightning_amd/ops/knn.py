"""K nearest neighbours and local feature smoothing: the SegAnyGS route's per-step smoothing and the search both it and the
appearance-similarity regulariser start from (include/gspl_hip.h section 19, csrc/knn.hip, csrc/smooth.hip).

  knn_points(p1, p2, lengths1=None, lengths2=None, K=1, version=-1, return_nn=False, return_sorted=True) -> (dists, idx, knn)
      `pytorch3d.ops.knn_points` for 3-D clouds: exact, ordered by (d^2, index), the same bits on every run.
  knn_graph(idx) -> KnnGraph
      a neighbour map [N, K] as int32 with its inverse adjacency in CSR form; built once per map.
  smooth_features(features, graph, columns=None) -> [N, D]
      normalise, mean over the selected neighbour columns, normalise (internal/segany_splatting.py:280-308) in one launch per
      direction; the [N, S, D] gather is never materialised and the backward uses no atomics.

GPU only, float32; no fallback."""
from __future__ import annotations

from collections import namedtuple

import torch
from torch import Tensor

from .. import _lib as L
from . import _args as A
from ._common import _guarded

MAX_K = 32
MAX_D = 128
_KNN = namedtuple("KNN", "dists idx knn")


@_guarded(0)
def _search(p1: Tensor, p2: Tensor, K: int, dists: Tensor, idx: Tensor):
    P1, P2 = p1.shape[0], p2.shape[0]
    ws_bytes = L.lib().gspl_knn_points_workspace_bytes(P2)
    if ws_bytes == 0:
        raise RuntimeError("gspl_knn_points_workspace_bytes failed: " + L.lib().gspl_last_error().decode())
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=p2.device)
    L.call("gspl_knn_points", P1, L.ptr(p1), P2, L.ptr(p2), K, L.ptr(dists), L.ptr(idx), L.ptr(ws), ws_bytes, L.stream())


def knn_points(p1: Tensor, p2: Tensor, lengths1=None, lengths2=None, K: int = 1, version: int = -1, return_nn: bool = False,
               return_sorted: bool = True):
    """`pytorch3d.ops.knn_points` as published, for what the reference calls it with (internal/segany_splatting.py:273,
    internal/metrics/appearance_feature_similarity_regularization_metrics.py:70-74): p1 [B, P1, 3], p2 [B, P2, 3] float32 on the GPU
    -> namedtuple (dists [B, P1, K] squared distances ascending, idx [B, P1, K] int64 into p2, knn [B, P1, K, 3] or None).

    Exact.  Neighbours are ordered by (d^2, index): among equal float32 d^2 the lower index comes first, and two calls on the same
    input return the same bits.  A query that coincides with a reference point finds it at distance 0 (with p1 is p2 every point is
    its own first neighbour).  Where P2 < K the trailing entries of dists and idx are zeros, as pytorch3d publishes; reference
    points with a non-finite coordinate are never returned, and the row of a non-finite query is zeros.  `version` is accepted and
    ignored; the result is always sorted.  If an input requires grad, dists is recomputed from idx with torch ops so that the
    gradient flows to p1 and p2 as in pytorch3d; the search itself is not differentiable.
    Not built (NotImplementedError): lengths1 / lengths2, a last dimension other than 3, K > 32.  CPU tensors raise RuntimeError.
    Parity with pytorch3d's own build is UNPINNED: there is no ROCm build of it to compare against; these are its published
    semantics, checked against an fp64 brute force."""
    if lengths1 is not None or lengths2 is not None:
        raise NotImplementedError("knn_points: lengths1 / lengths2 are not built (every cloud is used whole)")
    if p1.dim() != 3 or p2.dim() != 3 or p1.shape[0] != p2.shape[0]:
        raise ValueError(f"knn_points: p1 and p2 must be [B, P, 3] with one batch size, got {tuple(p1.shape)} and {tuple(p2.shape)}")
    if p1.shape[2] != 3 or p2.shape[2] != 3:
        raise NotImplementedError(f"knn_points: only 3-D points are built, got a last dimension of {p1.shape[2]} / {p2.shape[2]}")
    K = int(K)
    if K < 1:
        raise ValueError(f"knn_points: K must be at least 1, got {K}")
    if K > MAX_K:
        raise NotImplementedError(f"knn_points: K <= {MAX_K} is built, got {K}")
    A.on_gpu("knn_points", "p1", p1)
    A.on_gpu("knn_points", "p2", p2, p1, "p1")
    A.dtype("knn_points", "p1", p1, torch.float32, error=RuntimeError)
    A.dtype("knn_points", "p2", p2, torch.float32, error=RuntimeError)
    B, P1 = p1.shape[0], p1.shape[1]
    same = p1 is p2
    q = p1.detach().contiguous()
    r = q if same else p2.detach().contiguous()
    dists = torch.empty((B, P1, K), dtype=torch.float32, device=p1.device)
    idx = torch.empty((B, P1, K), dtype=torch.int64, device=p1.device)
    for b in range(B):
        _search(q[b], r[b], K, dists[b], idx[b])
    if p1.requires_grad or p2.requires_grad or return_nn:
        found = torch.stack([p2[b][idx[b]] for b in range(B)]) if p2.shape[1] > 0 else p2.new_zeros((B, P1, K, 3))
        if p1.requires_grad or p2.requires_grad:
            real = dists.new_ones(()) if p2.shape[1] >= K else (torch.arange(K, device=p1.device) < p2.shape[1]).to(dists.dtype)
            dists = ((p1[:, :, None, :] - found) ** 2).sum(-1) * real
        if return_nn and p2.shape[1] < K:
            found = found * (torch.arange(K, device=p1.device) < p2.shape[1]).to(found.dtype)[None, None, :, None]
    return _KNN(dists, idx, found if return_nn else None)


class KnnGraph:
    """A neighbour map and its transpose: idx [N, K] int32, and for every row j the positions e = i * K + k with idx[i, k] == j,
    ascending, as entries[row_start[j] : row_start[j + 1]] (both int32 tensors holding the unsigned values)."""
    __slots__ = ("idx", "row_start", "entries", "N", "K")

    def __init__(self, idx: Tensor, row_start: Tensor, entries: Tensor):
        self.idx, self.row_start, self.entries = idx, row_start, entries
        self.N, self.K = int(idx.shape[0]), int(idx.shape[1])

    def inverse(self, j: int):
        """The (i, k) pairs that reference row j, as an [n, 2] int64 tensor (for inspection and tests)."""
        lo, hi = int(self.row_start[j]), int(self.row_start[j + 1])
        e = self.entries[lo:hi].to(torch.int64)
        return torch.stack([e // self.K, e % self.K], dim=1)


@_guarded(0)
def _build_graph(idx32: Tensor) -> KnnGraph:
    N, K = idx32.shape
    dev = idx32.device
    row_start = torch.empty((N + 1,), dtype=torch.int32, device=dev)
    entries = torch.empty((N * K,), dtype=torch.int32, device=dev)
    ws_bytes = L.lib().gspl_knn_graph_workspace_bytes(N, K)
    if ws_bytes == 0:
        raise RuntimeError(f"knn_graph: a map of {N} x {K} is not supported (N * K < 2^30)")
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    L.call("gspl_knn_graph", N, K, L.ptr(idx32), L.ptr(row_start), L.ptr(entries), L.ptr(ws), ws_bytes, L.stream())
    return KnnGraph(idx32, row_start, entries)


@torch.no_grad()
def knn_graph(idx: Tensor) -> KnnGraph:
    """idx [N, K] (any integer type, values 0 .. N-1, 1 <= K <= 32) -> KnnGraph.  Built on the device (count, scan, stable radix
    sort): the inverse lists are sorted by (i, k), so the structure is the same on every run.  The values are checked here, once
    (one read-back), because `smooth_features` trusts them."""
    A.on_gpu("knn_graph", "idx", idx)
    if idx.dim() != 2 or idx.dtype.is_floating_point or idx.dtype == torch.bool:
        raise ValueError(f"knn_graph: idx must be an integer tensor [N, K], got {tuple(idx.shape)} {idx.dtype}")
    N, K = idx.shape
    if K < 1 or K > MAX_K:
        raise NotImplementedError(f"knn_graph: 1 <= K <= {MAX_K} is built, got {K}")
    if N > 0:
        lo, hi = (int(v) for v in torch.aminmax(idx))
        if lo < 0 or hi >= N:
            raise ValueError(f"knn_graph: idx must index its own rows (0 .. {N - 1}), found {lo} .. {hi}")
    return _build_graph(idx.to(torch.int32).contiguous())


def _column_mask(columns, K: int) -> int:
    if columns is None:
        return (1 << K) - 1
    cols = columns.reshape(-1).tolist() if isinstance(columns, Tensor) else [int(c) for c in columns]
    mask = 0
    for c in cols:
        c = int(c)
        if c < 0 or c >= K:
            raise ValueError(f"smooth_features: column {c} is outside 0 .. {K - 1}")
        mask |= 1 << c
    if mask == 0:
        raise ValueError("smooth_features: no column selected")
    return mask


class _SmoothFn(torch.autograd.Function):
    @staticmethod
    @_guarded(1)
    def forward(ctx, features, graph, mask):
        N, D = features.shape
        x = features.detach().contiguous()
        out = torch.empty_like(x)
        mnorm = torch.empty((N,), dtype=torch.float32, device=x.device)
        L.call("gspl_smooth_features_fwd", N, D, graph.K, mask, L.ptr(x), L.ptr(graph.idx), L.ptr(out), L.ptr(mnorm), L.stream())
        ctx.save_for_backward(x, out, mnorm)
        ctx.graph, ctx.mask = graph, mask
        return out

    @staticmethod
    @_guarded(0)
    def backward(ctx, v_out):
        x, out, mnorm = ctx.saved_tensors
        g = ctx.graph
        N, D = x.shape
        v = v_out.to(torch.float32).contiguous()
        v_x = torch.empty_like(x)
        L.call("gspl_smooth_features_bwd", N, D, g.K, ctx.mask, L.ptr(x), L.ptr(g.row_start), L.ptr(g.entries), L.ptr(out), L.ptr(mnorm),
               L.ptr(v), L.ptr(v_x), L.stream())
        return v_x, None, None


def smooth_features(features: Tensor, graph: KnnGraph, columns=None) -> Tensor:
    """The reference's local feature smoothing (internal/segany_splatting.py:280-308):
        n = F.normalize(features, dim=-1);  m_i = mean over the selected k of n[idx[i, k]];  out_i = m_i / (|m_i| + 1e-9)
    features [N, D] float32 on the GPU (1 <= D <= 128); graph = knn_graph(idx) of the same N; columns: the selected columns of idx
    (an int tensor or sequence, a subset of 0 .. K-1 — the reference's `torch.randperm(K)[:int(K * dropout)]`; a CPU tensor costs
    nothing, a device tensor one read-back), None = all K.  Differentiable in `features`; the backward is bit-reproducible."""
    if not isinstance(graph, KnnGraph):
        raise TypeError("smooth_features: graph must come from ops.knn_graph")
    A.dtype("smooth_features", "features", A.on_gpu("smooth_features", "features", features), torch.float32, error=RuntimeError)
    if features.dim() != 2 or features.shape[0] != graph.N:
        raise ValueError(f"smooth_features: features must be [{graph.N}, D], got {tuple(features.shape)}")
    if features.shape[1] < 1 or features.shape[1] > MAX_D:
        raise NotImplementedError(f"smooth_features: 1 <= D <= {MAX_D} is built, got {features.shape[1]}")
    A.on_gpu("smooth_features", "features", features, graph.idx, "the graph")
    return _SmoothFn.apply(features, graph, _column_mask(columns, graph.K))

"""SegAnyGS on the HIP ops: the per-step local feature smoothing of internal/segany_splatting.py:262-309.

The reference computes a K = 16 nearest-neighbour map of the Gaussian centres once (`pytorch3d.ops.knn_points`, :273) and then, every
step, normalises the per-Gaussian features, gathers a random half of each Gaussian's neighbours into an [N, 8, 32] tensor, takes the
mean and normalises again.  `HipFeatureSmoother` does the search with `ops.knn_points`, keeps the map with its inverse adjacency
(`ops.knn_graph`) and runs each step as one `ops.smooth_features` launch per direction.

    module = SegAnySplatting(...)                 # the reference's LightningModule, unedited (compat.install() provides pytorch3d.ops)
    use_hip_smoothing(module)                     # get_processed_semantic_features now runs on the fused op
"""
from __future__ import annotations

import types
from typing import Optional

import torch
from torch import Tensor

from . import ops


class HipFeatureSmoother:
    """`get_processed_semantic_features` of the reference as a callable: smoother(features, xyz, training, generator=None) -> [N, D].

    K, dropout: the reference's `smooth_K` and `smooth_dropout`.  In training with 0 < dropout < 1 each call draws
    `torch.randperm(K)[:int(K * dropout)]` (from `generator`, a CPU generator, when given) and averages those columns of the map;
    otherwise all K.  K <= 1 returns the features re-normalised (:265-266, :308).  The neighbour map is computed on the first call
    and again whenever K or the number of points changes; `reset()` drops it (after densification or pruning of a model whose size
    happens to stay the same)."""

    def __init__(self, K: int = 16, dropout: float = 0.5):
        self.K, self.dropout = int(K), float(dropout)
        self.graph: Optional[ops.KnnGraph] = None
        self.last_columns: Optional[Tensor] = None

    def reset(self):
        self.graph = None

    def _map(self, xyz: Tensor) -> "ops.KnnGraph":
        if self.graph is None or self.graph.K != self.K or self.graph.N != xyz.shape[0]:
            with torch.no_grad():
                pts = xyz.detach().to(torch.float32)
                found = ops.knn_points(pts.unsqueeze(0), pts.unsqueeze(0), K=self.K)
                self.graph = ops.knn_graph(found.idx[0])
        return self.graph

    def __call__(self, features: Tensor, xyz: Tensor, training: bool, generator: Optional[torch.Generator] = None) -> Tensor:
        if self.K <= 1:
            return features / (features.norm(dim=-1, keepdim=True) + 1e-9)
        dropout = self.dropout if training else -1.0
        assert dropout < 0 or int(self.K * dropout) >= 1
        columns = None
        if 0 < dropout < 1:
            columns = torch.randperm(self.K, generator=generator)[: int(self.K * dropout)]
        self.last_columns = columns
        return ops.smooth_features(features, self._map(xyz), columns)


def use_hip_smoothing(module, generator: Optional[torch.Generator] = None) -> HipFeatureSmoother:
    """Rebind `get_processed_semantic_features` of a `SegAnySplatting` instance (anything with `gaussian_semantic_features`,
    `models.gaussian.get_xyz`, `smooth_K`, `smooth_dropout` and `training`) to a `HipFeatureSmoother`, which is returned and kept on
    the module as `hip_feature_smoother`.  `smooth_K` and `smooth_dropout` are read at every call, as the reference reads them."""
    smoother = HipFeatureSmoother(getattr(module, "smooth_K", 16), getattr(module, "smooth_dropout", 0.5))

    def get_processed_semantic_features(self):
        smoother.K, smoother.dropout = int(self.smooth_K), float(self.smooth_dropout)
        return smoother(self.gaussian_semantic_features, self.models.gaussian.get_xyz, bool(self.training), generator)

    module.hip_feature_smoother = smoother
    module.get_processed_semantic_features = types.MethodType(get_processed_semantic_features, module)
    return smoother

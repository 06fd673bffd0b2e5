"""HipEnvLight — drop-in for the reference's `EnvLight` (internal/model_components/envlight.py): a learnable cube-map sky, sampled by
`ops.cubemap_sample` (csrc/envlight.hip) where the reference calls `nvdiffrast.torch.texture(..., filter_mode='linear',
boundary_mode='cube')`.  Same parameter name and shape (`base` [6, R, R, 3], initialised to 0.5), so the reference's checkpoints load.
The sampling rules are the published OpenGL / nvdiffrast ones (include/gspl_hip.h section 17); parity with nvdiffrast's own build is
unpinned."""
from __future__ import annotations

import torch

from . import ops


class HipEnvLight(torch.nn.Module):
    def __init__(self, resolution: int = 1024):
        super().__init__()
        self.base = torch.nn.Parameter(0.5 * torch.ones(6, resolution, resolution, 3, requires_grad=True))

    @staticmethod
    def to_opengl(l: torch.Tensor) -> torch.Tensor:
        """The reference's `l @ to_opengl.T`: (x, y, z) -> (x, z, -y)."""
        return torch.stack([l[..., 0], l[..., 2], -l[..., 1]], dim=-1)

    def forward(self, l: torch.Tensor) -> torch.Tensor:
        """World-space directions [..., 3] -> the sky's colour [..., 3]; the gradient reaches `base` (directions that require a
        gradient are refused by the op: there is none for them)."""
        return ops.cubemap_sample(self.base, self.to_opengl(l))

"""The `fused_bilagrid` interface the reference's bilateral-grid output processor imports (internal/output_processors/bilagrid.py:40,
`BilagridProcessor.fused = True`, the default of configs/bilagrid.yaml and configs/bilagrid_fused.yaml), on the HIP ops of
`gspl_amd.ops.bilagrid`.  `gspl_amd.compat` registers it as `fused_bilagrid` when that CUDA package is not importable.

  BilateralGrid(num, grid_X=16, grid_Y=16, grid_W=8)   `grids` [num, 12, grid_W, grid_Y, grid_X] initialised to the identity affine,
      and lib_bilagrid's persistent buffer `rgb2gray_weight`, so that checkpoints move both ways between this module and
      internal/utils/lib_bilagrid.py.  `tv_loss()`; `forward()` (the affine matrices, which nothing calls) raises NotImplementedError.
  slice(bil_grids, xy, rgb, grid_idx) -> {"rgb": ...}   4-D inputs (B, H, W, .); the 2-D and 3-D point forms raise NotImplementedError.
  total_variation_loss(x)                               on the 5-D grids."""
from __future__ import annotations

import torch
from torch import nn

MAX_GRID_W = 28                 # L: the kernels' bounds (include/gspl_hip.h section 14)
MAX_GRID_XY = 1024
MAX_GRID_VERTICES = 16384       # grid_W * grid_Y * grid_X


class BilateralGrid(nn.Module):
    def __init__(self, num: int, grid_X: int = 16, grid_Y: int = 16, grid_W: int = 8):
        super().__init__()
        if not (1 <= grid_W <= MAX_GRID_W and 1 <= grid_X <= MAX_GRID_XY and 1 <= grid_Y <= MAX_GRID_XY
                and grid_W * grid_X * grid_Y <= MAX_GRID_VERTICES):
            raise ValueError(f"bilateral grid {grid_X} x {grid_Y} x {grid_W}: supported are grid_W <= {MAX_GRID_W}, grid_X, grid_Y <= "
                             f"{MAX_GRID_XY} and grid_X * grid_Y * grid_W <= {MAX_GRID_VERTICES}")
        self.grid_width, self.grid_height, self.grid_guidance = grid_X, grid_Y, grid_W
        identity = torch.tensor([1., 0, 0, 0, 0, 1., 0, 0, 0, 0, 1., 0]).reshape(1, 12, 1, 1, 1)
        self.grids = nn.Parameter(identity.repeat(num, 1, grid_W, grid_Y, grid_X).contiguous())
        self.register_buffer("rgb2gray_weight", torch.tensor([[0.299, 0.587, 0.114]]))

    def tv_loss(self):
        return total_variation_loss(self.grids)

    def forward(self, *args, **kwargs):
        raise NotImplementedError("BilateralGrid.forward (the sliced affine matrices) is not provided; use slice(...)['rgb']")


def slice(bil_grids: BilateralGrid, xy, rgb, grid_idx):  # noqa: A001 (the package's name)
    if rgb.dim() != 4:
        raise NotImplementedError(f"slice: 4-D inputs (B, H, W, 3) only, got rgb of shape {tuple(rgb.shape)}")
    from . import ops
    return {"rgb": ops.bilagrid_slice(bil_grids.grids, xy, rgb, grid_idx)}


def total_variation_loss(x):
    if x.dim() != 5:
        raise NotImplementedError(f"total_variation_loss: the 5-D grids only, got shape {tuple(x.shape)}")
    from . import ops
    return ops.bilagrid_tv(x)

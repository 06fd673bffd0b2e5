"""F_theta of "SWAG: Splatting in the Wild images with Appearance-conditioned Gaussians" (arXiv 2403.10427) as the reference builds it
(internal/models/swag_model.py):   (c^I, delta alpha^I) = F_theta(c, emb(x), l_I)
with emb = the multiresolution hash grid of `gspl_amd.hashgrid.Encoding` (HIP), l_I an `nn.Embedding` row and F_theta a plain
`torch.nn` MLP (the reference's `NetworkFactory(tcnn=False)`).  The configuration dataclasses carry the reference's field names and
need nothing of the reference tree; the module's parameter names (`grid_encoding.params`, `image_embedding.weight`, `theta.<i>.*`)
are the reference's, so that its checkpoints load.

One deliberate difference: `GridEncodingConfig.n_levels` defaults to 12, the value the reference writes down (swag_model.py:18).
There the line lacks its annotation, so the inherited dataclass field keeps 8 and an unconfigured reference run trains 8 levels with
per_level_scale 2; pass `n_levels=8` to read such a checkpoint."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Union

import torch
from torch import nn

from .hashgrid import Encoding


@dataclass
class GridEncodingConfig:
    """The reference's `TCNNEncodingConfig` fields (internal/configs/tcnn_encoding_config.py); only the grid types are built."""
    type: str = "hashgrid"          # "hashgrid" | "densegrid"
    n_frequencies: int = 4          # (frequency / SphericalHarmonics encodings: not built)
    degree: int = 4
    n_features_per_level: int = 4
    log2_hashmap_size: int = 19
    max_resolution: int = 2048
    n_levels: int = 12
    base_resolution: int = 16
    per_level_scale: float = 1.405

    def get_encoder_config(self, n_input_channels: int) -> dict:
        if self.type == "hashgrid":
            growth = math.exp((math.log(self.max_resolution) - math.log(self.base_resolution)) / (self.n_levels - 1)) if self.n_levels > 1 else 1
            return {"n_dims_to_encode": n_input_channels, "otype": "HashGrid", "n_levels": self.n_levels,
                    "n_features_per_level": self.n_features_per_level, "log2_hashmap_size": self.log2_hashmap_size,
                    "base_resolution": self.base_resolution, "per_level_scale": growth}
        if self.type == "densegrid":
            return {"n_dims_to_encode": n_input_channels, "otype": "DenseGrid", "n_levels": self.n_levels,
                    "base_resolution": self.base_resolution, "per_level_scale": self.per_level_scale}
        raise NotImplementedError(f"GridEncodingConfig: type {self.type!r} is not built (hashgrid and densegrid are)")


@dataclass
class NetworkConfig:
    n_neurons: int = 64
    n_layers: int = 3


@dataclass
class EmbeddingConfig:
    num_embeddings: int = 2048
    embedding_dim: int = 24


@dataclass
class GridEncodingOptimizationConfig:
    lr: float = 1e-3
    max_steps: int = 30_000
    lr_final_factor: float = 0.01
    eps: float = 1e-15


def mlp(n_input_dims: int, n_output_dims: int, n_layers: int, n_neurons: int) -> nn.Sequential:
    """The reference's `NetworkFactory(tcnn=False).get_network(..., activation="ReLU", output_activation="None")`."""
    assert n_layers > 0 and n_neurons > 0
    layers, width = [], n_input_dims
    for _ in range(n_layers - 1):
        layers += [nn.Linear(width, n_neurons), nn.ReLU()]
        width = n_neurons
    layers.append(nn.Linear(width, n_output_dims))
    return nn.Sequential(*layers)


class HipSWAGModel(nn.Module):
    def __init__(self, network: NetworkConfig = NetworkConfig(), grid_encoding: GridEncodingConfig = GridEncodingConfig(),
                 embedding: EmbeddingConfig = EmbeddingConfig()) -> None:
        super().__init__()
        self.network_config = network
        self.grid_encoding_config = grid_encoding
        self.embedding_config = embedding
        self.grid_encoding = Encoding(n_input_dims=3, encoding_config=self.grid_encoding_config.get_encoder_config(3))
        self.image_embedding = nn.Embedding(self.embedding_config.num_embeddings, self.embedding_config.embedding_dim)
        self.theta = mlp(self.grid_encoding.n_output_dims + self.embedding_config.embedding_dim + 3, 4,      # 3: c^I, 1: delta alpha^I
                         self.network_config.n_layers, self.network_config.n_neurons)
        self._image_ids: dict = {}

    def _image_id(self, image_id: Union[int, torch.Tensor], device) -> torch.Tensor:
        if isinstance(image_id, torch.Tensor):          # stays on its device: no read-back
            return image_id.reshape(1).to(device=device, dtype=torch.int)
        key = (int(image_id), device)
        found = self._image_ids.get(key)
        if found is None:
            found = self._image_ids[key] = torch.tensor([int(image_id)], dtype=torch.int, device=device)
        return found

    def forward(self, colors: torch.Tensor, x: torch.Tensor, image_id: Union[int, torch.Tensor]):
        """colors [n, 3], x [n, 3] normalised means, image_id -> (c^I [n, 3], delta alpha^I [n]); the arithmetic of swag_model.py:98-105."""
        x_emb = self.grid_encoding(x).to(colors.dtype)
        image_emb = self.image_embedding(self._image_id(image_id, colors.device)).expand(colors.shape[0], -1)
        output = self.theta(torch.concat([colors, x_emb, image_emb], dim=-1))
        return torch.sigmoid(output[:, :3]), output[:, -1]

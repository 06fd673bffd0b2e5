"""The appearance model of the reference's `GSplatAppearanceEmbeddingRenderer` (internal/renderers/gsplat_appearance_embedding_renderer.py:
18-93):   colour offsets (and an opacity offset) = MLP([Gaussian features | appearance embedding | encoded view direction]).
The configuration dataclasses carry the reference's field names and defaults and need nothing of the reference tree; the module's
parameter names (`embedding.weight`, `network.output_layers.<i>.*`, `network.skip_layers.<s>.<i>.*`) are the reference's, so that
its checkpoints load unchanged.

Two paths over the SAME parameters:
  * `ops.appearance_mlp` (one HIP launch forward, one launch and an ordered reduce backward) when the configuration is built and
    `fused_mlp` is on;
  * torch.nn.functional in the reference's order of operations otherwise (skip layers, other widths, CPU tensors), so that every
    configuration of the reference runs.
`tcnn: true` is accepted, warned about once, and means the same fp32 path: there is no half-precision network here."""
from __future__ import annotations

import warnings
from dataclasses import dataclass, field
from typing import List, Optional

import torch
import torch.nn.functional as F
from torch import nn

from .ops import appearance as _op


@dataclass
class ModelConfig:
    n_gaussian_feature_dims: int = 64
    n_appearances: int = -1
    n_appearance_embedding_dims: int = 32
    is_view_dependent: bool = False
    n_view_direction_frequencies: int = 4
    n_neurons: int = 64
    n_layers: int = 3
    skip_layers: List[int] = field(default_factory=lambda: [])
    with_opacity: bool = False
    normalize: bool = False
    tcnn: bool = False
    """Accepted for the reference's configuration files; the network is fp32 either way."""


@dataclass
class OptimizationConfig:
    gamma_eps: float = 1e-6
    embedding_lr_init: float = 2e-3
    embedding_lr_final_factor: float = 0.1
    lr_init: float = 1e-3
    lr_final_factor: float = 0.1
    eps: float = 1e-15
    max_steps: int = 30_000
    warm_up: int = 4000


def _sequential(n_input_dims: int, n_output_dims: int, n_layers: int, n_neurons: int, output_activation: Optional[nn.Module]) -> nn.Sequential:
    """n_layers Linear layers, ReLU between them, `output_activation` (or nothing) after the last: even indices are the Linears."""
    assert n_layers > 0 and n_neurons > 0
    modules, width = [], n_input_dims
    for _ in range(n_layers - 1):
        modules += [nn.Linear(width, n_neurons), nn.ReLU()]
        width = n_neurons
    modules.append(nn.Linear(width, n_output_dims))
    if output_activation is not None:
        modules.append(output_activation)
    return nn.Sequential(*modules)


class SkipNetwork(nn.Module):
    """`skip_layers`: groups of layers whose output is concatenated with the network's input before the next group; then
    `output_layers`.  Without skips only `output_layers` exists (keys network.output_layers.{0,2,4}.* for three layers)."""

    def __init__(self, n_input_dims: int, n_output_dims: int, n_layers: int, n_neurons: int, skips: List[int]):
        super().__init__()
        groups, done, width = [], 0, n_input_dims
        for at in skips:
            groups.append(_sequential(width, n_neurons, at - done, n_neurons, nn.ReLU()))
            width = n_neurons + n_input_dims
            done = at
        self.skip_layers = nn.ModuleList(groups)
        self.output_layers = _sequential(width, n_output_dims, n_layers - done, n_neurons, nn.Sigmoid())

    def forward(self, x):
        value = x
        for group in self.skip_layers:
            value = torch.concat([x, group(value)], dim=-1)
        return self.output_layers(value)


_TCNN_WARNED = False


def view_direction_encoding(d: torch.Tensor, n_frequencies: int) -> torch.Tensor:
    """x, sin(2^0 x), cos(2^0 x), sin(2^1 x), ... (internal/encodings/positional_encoding.py:35-40, log sampling)."""
    bands = 2. ** torch.linspace(0., n_frequencies - 1, steps=n_frequencies)
    parts = [d]
    for band in bands:
        parts += [torch.sin(band * d), torch.cos(band * d)]
    return torch.cat(parts, -1)


class HipAppearanceModel(nn.Module):
    def __init__(self, config: ModelConfig, fused_mlp: bool = True):
        super().__init__()
        global _TCNN_WARNED
        self.config = config
        self.fused_mlp = bool(fused_mlp)
        if config.tcnn and not _TCNN_WARNED:
            _TCNN_WARNED = True
            warnings.warn("appearance model: `tcnn: true` has no half-precision network here; the fp32 path runs")
        self.n_output_dims = 4 if config.with_opacity else 3
        self.embedding = nn.Embedding(num_embeddings=config.n_appearances, embedding_dim=config.n_appearance_embedding_dims)
        self.n_encoding_dims = _op.view_encoding_dims(config.n_view_direction_frequencies) if config.is_view_dependent else 0
        n_input_dims = config.n_gaussian_feature_dims + config.n_appearance_embedding_dims + self.n_encoding_dims
        self.network = SkipNetwork(n_input_dims, self.n_output_dims, config.n_layers, config.n_neurons, list(config.skip_layers))
        self._ids: dict = {}

    def _appearance_index(self, appearance, device) -> torch.Tensor:
        if isinstance(appearance, torch.Tensor):          # stays on its device: no read-back
            return appearance.reshape((-1,))
        key = (int(appearance), device)
        found = self._ids.get(key)
        if found is None:
            found = self._ids[key] = torch.tensor([int(appearance)], dtype=torch.int, device=device)
        return found

    def unbuilt_reason(self) -> Optional[str]:
        """None when `ops.appearance_mlp` is built for this configuration, else the refusal's text."""
        c = self.config
        try:
            _op.appearance_mlp_check(c.n_gaussian_feature_dims, c.n_appearance_embedding_dims, c.n_neurons, c.n_layers, self.n_output_dims,
                                     c.n_view_direction_frequencies if c.is_view_dependent else 0, "sigmoid", c.skip_layers,
                                     self.embedding.weight.dtype)
        except NotImplementedError as e:
            return str(e)
        return None

    def uses_fused(self, features: torch.Tensor) -> bool:
        return self.fused_mlp and features.is_cuda and self.unbuilt_reason() is None

    def _linears(self):
        return [m for m in self.network.output_layers if isinstance(m, nn.Linear)]

    def forward(self, gaussian_features, appearance, view_dirs=None, *, mask=None, means=None, camera_center=None):
        """gaussian_features [n, F], appearance: the id (a tensor, it stays on its device), and for a view-dependent model either
        `view_dirs` [n, 3] (unit directions, the reference's call) or `means` [n, 3] with `camera_center` [3].  mask [n] bool or None:
        rows it drops come back as zeros and get no gradient.  -> [n, n_output_dims]."""
        c = self.config
        n = gaussian_features.shape[0]
        if n == 0:
            return torch.zeros((0, self.n_output_dims), dtype=gaussian_features.dtype, device=gaussian_features.device)
        embedding = self.embedding(self._appearance_index(appearance, gaussian_features.device))
        if c.is_view_dependent and means is None:
            means, camera_center = view_dirs, torch.zeros((3,), dtype=view_dirs.dtype, device=view_dirs.device)
        if self.uses_fused(gaussian_features):
            linears = self._linears()
            return _op.appearance_mlp(gaussian_features, [m.weight for m in linears], [m.bias for m in linears], embedding[0], mask=mask,
                                      means=means if c.is_view_dependent else None, camera_center=camera_center if c.is_view_dependent else None,
                                      n_view_frequencies=c.n_view_direction_frequencies if c.is_view_dependent else 0,
                                      normalize=c.normalize, output_activation="sigmoid")
        # the reference's order of operations (gsplat_appearance_embedding_renderer.py:85-93)
        embeddings = embedding.repeat(n, 1)
        if c.normalize:
            gaussian_features = F.normalize(gaussian_features, dim=-1)
            embeddings = F.normalize(embeddings, dim=-1)
        inputs = [gaussian_features, embeddings]
        if c.is_view_dependent:
            if view_dirs is None:
                view_dirs = F.normalize(means.detach() - camera_center, dim=-1)
            inputs.append(view_direction_encoding(view_dirs, c.n_view_direction_frequencies))
        out = self.network(torch.concat(inputs, dim=-1))
        if mask is not None:
            out = torch.where(mask.unsqueeze(-1), out, torch.zeros((), dtype=out.dtype, device=out.device))
        return out

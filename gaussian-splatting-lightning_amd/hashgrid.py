"""`tinycudann.Encoding` for grid encodings, on `ops.hashgrid_encode` (include/gspl_hip.h section 20): what the SWAG route's model
builds (internal/models/swag_model.py:75-78) and `compat.install()` registers as `tinycudann` when that package is missing.

Built: otype `HashGrid`, `DenseGrid`, and `Grid` with `type` `Hash` / `Dense`; linear interpolation; float32 table and output.
Everything else of tiny-cuda-nn (other encodings, `Network`, `NetworkWithInputEncoding`, half-precision tables, Smoothstep /
Nearest interpolation, Tiled grids) is NOT built: an option that asks for it raises NotImplementedError naming it.  Parity with
tiny-cuda-nn's own build is UNPINNED; tests/hashgrid_oracle.py pins the published rules."""
from __future__ import annotations

import torch
from torch import nn

from . import ops

# tiny-cuda-nn's documented defaults of a grid encoding
_DEFAULTS = {"n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 2.0,
             "interpolation": "Linear"}
_IGNORED = ("otype", "type", "n_dims_to_encode")


class Encoding(nn.Module):
    """Encoding(n_input_dims, encoding_config, seed=1337, dtype=None): `.params` (flat float32 nn.Parameter, uniform in
    [-1e-4, 1e-4] from `seed`), `.n_input_dims`, `.n_output_dims` = n_levels * n_features_per_level, `forward(x [N, n_input_dims])`
    -> float32 [N, n_output_dims].  The table is created on the GPU when there is one."""

    def __init__(self, n_input_dims: int, encoding_config: dict, seed: int = 1337, dtype=None):
        super().__init__()
        config = dict(encoding_config)
        otype = str(config.get("otype", ""))
        kind = otype.lower()
        if kind == "grid":
            grid_type = str(config.get("type", "Hash"))
            if grid_type.lower() not in ("hash", "dense"):
                raise NotImplementedError(f"tinycudann.Encoding: Grid type {grid_type!r} is not built (Hash and Dense are)")
            dense = grid_type.lower() == "dense"
        elif kind in ("hashgrid", "densegrid"):
            dense = kind == "densegrid"
        else:
            raise NotImplementedError(f"tinycudann.Encoding: otype {otype!r} is not built (HashGrid, DenseGrid and Grid are)")
        unknown = sorted(set(config) - set(_DEFAULTS) - set(_IGNORED))
        if unknown:
            raise NotImplementedError(f"tinycudann.Encoding: option(s) {unknown} are not built")
        if int(config.get("n_dims_to_encode", n_input_dims)) != int(n_input_dims):
            raise NotImplementedError(f"tinycudann.Encoding: n_dims_to_encode {config['n_dims_to_encode']} differs from n_input_dims "
                                      f"{n_input_dims}; encoding a part of the input is not built")
        settings = {**_DEFAULTS, **{k: v for k, v in config.items() if k in _DEFAULTS}}
        if str(settings["interpolation"]).lower() != "linear":
            raise NotImplementedError(f"tinycudann.Encoding: interpolation {settings['interpolation']!r} is not built (Linear is)")
        if dtype not in (None, torch.float32):
            raise NotImplementedError(f"tinycudann.Encoding: dtype {dtype} is not built (the table and the output are float32)")
        self.n_input_dims = int(n_input_dims)
        self.encoding_config = config
        self.seed = int(seed)
        self.dtype = torch.float32
        self.levels = ops.hashgrid_levels(self.n_input_dims, settings["n_levels"], settings["n_features_per_level"],
                                          settings["log2_hashmap_size"], settings["base_resolution"], settings["per_level_scale"], dense=dense)
        self.n_output_dims = self.levels.n_output_dims
        device = "cuda" if torch.cuda.is_available() else None
        self.params = nn.Parameter(ops.hashgrid_table(self.levels, self.seed, device))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.hashgrid_encode(x, self.params, self.levels)

    def extra_repr(self) -> str:
        return f"n_input_dims={self.n_input_dims}, n_output_dims={self.n_output_dims}, seed={self.seed}, config={self.encoding_config}"

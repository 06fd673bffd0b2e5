"""
make_hexplane_golden.py — generates tests/golden/ref_hexplane.npz and tests/golden/gs4d_state_keys.json by IMPORTING the reference's own
torch code (internal/model_components/gs4d_hexplane.py, gs4d_deformation.py) where its tree is present.

Run from the repo root:   python tests/golden/make_hexplane_golden.py <path to the reference tree>
Its outputs are committed; nothing under tests/ reads the reference tree at test time.

Fixtures
  ref_hexplane.npz       a seeded `HexPlaneField` in double precision (resolution [5, 6, 7, 3], multires [1, 2], 8 features, bounds 2.0;
                         every plane re-drawn from a seeded normal, so that the time planes are not the constant 1 they start as), 64
                         points of which half lie outside the box, per-point times in [-1.25, 1.25], and its output; then ONE forward of
                         `deform_network` at width 16 on that field with every deformation switched on: the state dict (as float64),
                         the five inputs and the five outputs
  gs4d_state_keys.json   the names and shapes of `deform_network(<the 4DGaussians default arguments>).state_dict()`
"""
import json
import os
import sys
from argparse import Namespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def default_args(**overrides):
    """`ModelHiddenParams` of 4DGaussians (arguments/__init__.py), the fields the deformation network reads."""
    args = dict(net_width=64, timebase_pe=4, defor_depth=1, posebase_pe=10, scale_rotation_pe=2, opacity_pe=2, timenet_width=64,
                timenet_output=32, bounds=1.6, grid_pe=0,
                kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 32, "resolution": [64, 64, 64, 25]},
                multires=[1, 2, 4, 8], no_dx=False, no_grid=False, no_ds=False, no_dr=False, no_do=True, no_dshs=True,
                empty_voxel=False, static_mlp=False, apply_rotation=False)
    args.update(overrides)
    return Namespace(**args)


def main(reference):
    sys.path.insert(0, reference)
    from internal.model_components.gs4d_deformation import deform_network

    keys = {name: list(value.shape) for name, value in deform_network(default_args()).state_dict().items()}
    with open(os.path.join(HERE, "gs4d_state_keys.json"), "w") as f:
        json.dump(keys, f, indent=1)
        f.write("\n")

    torch.manual_seed(20240)
    args = default_args(net_width=16, bounds=2.0, multires=[1, 2], no_do=False, no_dshs=False,
                        kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 8, "resolution": [5, 6, 7, 3]})
    net = deform_network(args).double()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for grids in net.deformation_net.grid.grids:
            for plane in grids:
                plane.copy_(torch.randn(plane.shape, generator=g, dtype=torch.float64))
    N = 64
    x = (torch.rand(N, 3, generator=g, dtype=torch.float64) * 2 - 1) * 1.9
    x[N // 2:] = x[N // 2:] * 2.5                                   # far outside ...
    x[N // 2:, 0] = torch.where(x[N // 2:, 0] > 0, 2.0, -2.0) + x[N // 2:, 0]      # ... every one of them at least along x
    t = (torch.rand(N, 1, generator=g, dtype=torch.float64) * 2 - 1) * 1.25
    assert int(((x.abs() > 2.0).any(dim=1)).sum()) == N // 2
    scales = torch.randn(N, 3, generator=g, dtype=torch.float64) - 3
    rotations = torch.nn.functional.normalize(torch.randn(N, 4, generator=g, dtype=torch.float64), dim=-1)
    opacity = torch.randn(N, 1, generator=g, dtype=torch.float64)
    shs = torch.randn(N, 16, 3, generator=g, dtype=torch.float64)
    with torch.no_grad():
        field = net.deformation_net.grid(x, t)
        outs = net(x, scales, rotations, opacity, shs, t)
    data = {"x": x, "t": t, "field": field, "in_scales": scales, "in_rotations": rotations, "in_opacity": opacity, "in_shs": shs}
    data.update({"out_" + n: o for n, o in zip(("means", "scales", "rotations", "opacity", "shs"), outs)})
    data.update({"state/" + n: v for n, v in net.state_dict().items()})
    np.savez_compressed(os.path.join(HERE, "ref_hexplane.npz"), **{k: v.numpy() for k, v in data.items()})
    print("wrote ref_hexplane.npz", os.path.getsize(os.path.join(HERE, "ref_hexplane.npz")), "bytes and gs4d_state_keys.json,", len(keys), "names")


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "internal", "model_components")):
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))

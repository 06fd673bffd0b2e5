"""
make_lod_golden.py — generates tests/golden/ref_lod.npz by IMPORTING the reference's own `PartitionLoDRendererModule`
(internal/renderers/partition_lod_renderer.py) where its tree is present and calling its unedited `get_partition_distances` in
float64, then applying the level rule of its `forward` (lines 553-557) as written there.

The reference module imports `pytorch3d` and `viser` when it is loaded; neither is needed by the method called here, so module objects
that hold only the imported names stand in for the two (and tests/lightning_standin.py for `lightning`, as in the other workers).

Run from the repo root:   python tests/golden/make_lod_golden.py <path to the reference tree>
Its output is committed; no test runs this script.

Fixture (ref_lod.npz), every input a float32 value stored as float64
  transform [3, 3]       a rotation (the reference's `orientation_transform`, already transposed as it keeps it)
  box_min, box_max [P, 2]   a 6 x 5 grid of partitions of size 2, P = 30
  thresholds [3]         0.75, 2.5, 6.0  (L = 4)
  cameras [C, 3]         C = 12 camera centres: inside the grid, outside it, far away, and one on a box edge
  distances [C, P]       `get_partition_distances(camera)`
  lods [C, P] int64      the level rule: fill with -1, then for i = L - 2 .. 0: lods[distances < thresholds[i]] = i; -1 taken modulo L
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)


def stand_in(name, **names):
    module = types.ModuleType(name)
    for k, v in names.items():
        setattr(module, k, v)
    sys.modules[name] = module
    return module


def main(reference):
    for p in (reference, TESTS, ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    import lightning_standin
    lightning_standin.install()
    import gspl_amd  # noqa: F401
    from gspl_amd import renderers  # noqa: F401   (installs the stand-ins of gspl_amd.compat)
    stand_in("pytorch3d")
    stand_in("pytorch3d.ops")
    stand_in("pytorch3d.ops.iou_box3d", _check_coplanar=None, _check_nonzero=None, _box3d_overlap=None)
    stand_in("viser", GuiMarkdownHandle=None, ViserServer=None, GuiEvent=None)
    from internal.renderers.partition_lod_renderer import PartitionLoDRendererModule

    g = torch.Generator().manual_seed(20261)
    q = torch.nn.functional.normalize(torch.randn(4, generator=g), dim=0)
    w, x, y, z = q.tolist()
    transform = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                              [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                              [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float32)
    ij = torch.stack(torch.meshgrid(torch.arange(6), torch.arange(5), indexing="ij"), -1).reshape(-1, 2).float()
    box_min = ij * 2.0 - torch.tensor([6.0, 5.0])
    box_max = box_min + 2.0
    thresholds = torch.tensor([0.75, 2.5, 6.0])
    cameras = torch.cat([torch.rand(6, 3, generator=g) * 12 - 6, torch.rand(4, 3, generator=g) * 60 - 30,
                         torch.tensor([[500.0, -300.0, 40.0]]), (torch.tensor([[-6.0, 1.0, 0.25]]) @ transform.T)])

    module = types.SimpleNamespace(orientation_transform=transform.double(),
                                   partition_bounding_boxes=types.SimpleNamespace(min=box_min.double(), max=box_max.double()))
    L = thresholds.numel() + 1
    distances, lods = [], []
    for c in cameras.double():
        d = PartitionLoDRendererModule.get_partition_distances(module, c)
        lod = torch.ones(d.shape[0], dtype=torch.int8).fill_(-1)
        for i in range(L - 2, -1, -1):
            lod[d < thresholds.double()[i]] = i
        distances.append(d)
        lods.append(lod.long() % L)
    out = {"transform": transform, "box_min": box_min, "box_max": box_max, "thresholds": thresholds, "cameras": cameras}
    out = {k: v.double().numpy() for k, v in out.items()}
    out["distances"] = torch.stack(distances).numpy()
    out["lods"] = torch.stack(lods).numpy()
    counts = np.bincount(out["lods"].reshape(-1), minlength=L)
    print("levels chosen:", counts.tolist(), "zero distances:", int((out["distances"] == 0).sum()))
    assert counts.min() > 0 and (out["distances"] == 0).any()
    path = os.path.join(HERE, "ref_lod.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])

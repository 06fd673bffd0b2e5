"""Writes tests/golden/ref_bilagrid.npz: the reference's own internal/utils/lib_bilagrid.py (`slice`, `total_variation_loss`, fp32,
CPU) on seeded cases, with the gradients of a seeded linear loss.  lib_bilagrid imports `tensorly` at the top for its CP-4D class
only; a stand-in module is registered for that import.

    python tests/golden/make_bilagrid_golden.py [reference root]

Cases (key prefix cN_): identity and random grids; colours outside [0, 1] and with gray exactly 0 and 1; B = 2 with distinct indices
and with one shared index; images 1 x 1, 1 x 17, 13 x 1, 37 x 23; grids 16 x 16 x 8 and 8 x 8 x 4.  TV at N = 1 and 3 (tvN_)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _stub_tensorly():
    tl = types.ModuleType("tensorly")
    tl.set_backend = lambda name: None
    dec = types.ModuleType("tensorly.decomposition")

    def parafac(*a, **k):
        raise NotImplementedError("tensorly stand-in: only the import is provided")
    dec.parafac = parafac
    tl.decomposition = dec
    sys.modules.setdefault("tensorly", tl)
    sys.modules.setdefault("tensorly.decomposition", dec)


# (B, H, W, (grid_X, grid_Y, grid_W), N, grid_idx, identity grid)
CASES = [
    (1, 13, 1, (16, 16, 8), 1, [[0]], True),
    (2, 37, 23, (16, 16, 8), 1, [[0]], False),          # B = 2 sharing one index
    (2, 1, 17, (8, 8, 4), 3, [[2], [0]], False),        # B = 2, distinct indices
    (1, 1, 1, (8, 8, 4), 3, [[1]], False),
]


def main(ref_root):
    sys.path.insert(0, ref_root)
    _stub_tensorly()
    from internal.utils import lib_bilagrid as lib
    out = {}
    for n, (B, H, W, (gx, gy, gw), N, gi, ident) in enumerate(CASES):
        g = torch.Generator().manual_seed(100 + n)
        bg = lib.BilateralGrid(N, grid_X=gx, grid_Y=gy, grid_W=gw)
        if not ident:
            with torch.no_grad():
                bg.grids.add_(0.3 * torch.randn(bg.grids.shape, generator=g))
        rgb = -0.25 + 1.5 * torch.rand(B, H, W, 3, generator=g)
        flat = rgb.view(B, -1, 3)
        if flat.shape[1] >= 3:
            flat[:, 0] = 0.0                              # gray exactly 0
            flat[:, 1] = 1.0                              # gray 1 (up to the rounding of the weights' sum)
        ys, xs = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
        xy = torch.stack([xs, ys], dim=-1).unsqueeze(0).expand(B, H, W, 2).contiguous()
        rgb.requires_grad_(True)
        idx = torch.tensor(gi)
        res = lib.slice(bg, xy, rgb, idx)["rgb"]
        w = torch.randn(res.shape, generator=g)
        (res * w).sum().backward()
        p = f"c{n}_"
        out.update({p + "grids": bg.grids.detach().numpy(), p + "xy": xy.numpy(), p + "rgb": rgb.detach().numpy(), p + "idx": idx.numpy(),
                    p + "dout": w.numpy(), p + "out": res.detach().numpy(), p + "grad_grids": bg.grids.grad.numpy(),
                    p + "grad_rgb": rgb.grad.numpy()})
    for N, (gx, gy, gw) in ((1, (16, 16, 8)), (3, (8, 8, 4))):
        g = torch.Generator().manual_seed(200 + N)
        x = (0.5 * torch.randn(N, 12, gw, gy, gx, generator=g)).requires_grad_(True)
        tv = lib.total_variation_loss(x)
        tv.backward()
        out.update({f"tv{N}_x": x.detach().numpy(), f"tv{N}_value": np.float32(tv.item()), f"tv{N}_grad": x.grad.numpy()})
    path = os.path.join(HERE, "ref_bilagrid.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GSPL_REFERENCE_ROOT", "/root/reference"))

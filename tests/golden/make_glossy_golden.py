"""
make_glossy_golden.py — generates tests/golden/ref_glossy.npz by IMPORTING the reference's own `eval_sh_decomposed`
(internal/utils/sh_utils.py) where its tree is present, and running in float64 exactly the expression of
`GlossyRendererModule.get_opacities` / `GlossyGaussianModel.get_view_dep_opacities`:
    F.normalize(means - camera, dim=-1) -> eval_sh_decomposed(degree, dc, rest, d) + 0.5 -> clamp(min=0, max=1)

Run from the repo root:   python tests/golden/make_glossy_golden.py <path to the reference tree>
Its output is committed; no test runs this script.

Fixture (ref_glossy.npz), N = 384 rows, every input a float32 value stored as float64
  means [N, 3]      uniform in [-1, 1]^3; row 7 equals the camera (the zero direction)
  camera [3]        (0.1, -0.2, 0.3)
  dc [N, 1, 1]      1.5 randn; dc[7] = 0
  rest [N, 24, 1]   0.5 randn (the full width of degree 4; lower degrees read its first columns)
  w [N]             randn: the weights of the scalar sum_n w_n opacity_n
  raw{deg}, value{deg} [N]                the value before and after the clamp, degrees 0 .. 4
  v_dc{deg} [N, 1, 1], v_rest{deg} [N, 24, 1]   autograd's gradients of that scalar
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
N, KR = 384, 24


def main(reference):
    sys.path.insert(0, reference)
    from internal.utils.sh_utils import eval_sh_decomposed

    g = torch.Generator().manual_seed(20251)
    camera = torch.tensor([0.1, -0.2, 0.3], dtype=torch.float32)
    means = torch.rand(N, 3, generator=g) * 2 - 1
    dc = 1.5 * torch.randn(N, 1, 1, generator=g)
    rest = 0.5 * torch.randn(N, KR, 1, generator=g)
    w = torch.randn(N, generator=g)
    means[7], dc[7] = camera, 0.0
    out = {"means": means, "camera": camera, "dc": dc, "rest": rest, "w": w}
    out = {k: v.double().numpy() for k, v in out.items()}
    for degree in range(5):
        dc64, rest64 = dc.double().requires_grad_(True), rest.double().requires_grad_(True)
        d = torch.nn.functional.normalize(means.double() - camera.double(), dim=-1)
        raw = (eval_sh_decomposed(degree, dc64, rest64, d) + 0.5).squeeze(-1)
        value = torch.clamp(raw, min=0., max=1.)
        (w.double() * value).sum().backward()
        v_rest = rest64.grad if rest64.grad is not None else torch.zeros_like(rest64)
        raw = raw.detach()
        out.update({f"raw{degree}": raw.numpy(), f"value{degree}": value.detach().numpy(), f"v_dc{degree}": dc64.grad.numpy(),
                    f"v_rest{degree}": v_rest.numpy()})
        below, above = float((raw < 0).double().mean()), float((raw > 1).double().mean())
        print(f"degree {degree}: below 0 {below:.3f}, interior {1 - below - above:.3f}, above 1 {above:.3f}; row 7 raw {float(raw[7]):.6f}")
        assert min(below, above, 1 - below - above) >= 0.10 and 0 < float(raw[7]) < 1
    path = os.path.join(HERE, "ref_glossy.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])

"""
make_mip_golden.py — generates tests/golden/ref_mip.npz by IMPORTING the reference's own, unedited `MipSplattingUtils`
(internal/models/mip_splatting.py) where its tree is present, and running it in float32 on the CPU, as the reference does.

Run from the repo root:   python tests/golden/make_mip_golden.py <path to the reference tree>
Its output is committed (inputs and recorded results only); no test runs this script.

`compute_3d_filter` returns the filter alone.  Its per-row distance and validity are recorded by OBSERVING the run: a
`TorchFunctionMode` copies the `distance` tensor after each of the function's own masked assignments (the last but one is the state
before the fill) and keeps the result of its last `torch.logical_or` (`valid_points`).  Nothing of the function is restated here.

Fixture (ref_mip.npz), float32 unless noted
  means [4160, 3]      4096 points uniform in [-1.5, 1.5]^3, then 64 (1.5 %) that no camera sees: 60 .. 70 above every frustum
  table [12, 16]       per camera R (row-major), T, fx, fy, width, height: ten cameras on a ring of radius 3 at height 0.4 looking at
                       the origin, two inside the cloud; 640 x 480 and 800 x 600 alternating; fx = 500 + 20 i, fy = fx + 7
  filter [4160, 1], distance [4160] (before the fill), valid_any [4160] bool
  a_scales [4099, 3] (activated: exp(randn - 4)), a_opacities [4099, 1] (sigmoid(2 randn)), a_filter [4099, 1] (0.001 .. 0.051),
  a_vs [4099, 3], a_vo [4099] (randn: the weights of the scalar sum vs * scales_out + sum vo * second)
  on{0,1}_opacities [4099, 1], on{0,1}_scales [4099, 3], on{0,1}_g_scales, on{0,1}_g_opacities   `apply_3d_filter` with
                       opacity_compensation = False / True, and autograd's gradients of the scalar
  sc_scales, sc_coef [4099], sc_g_scales            `apply_3d_filter_on_scales`
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
N_SEEN, N_HIDDEN, N_APPLY = 4096, 64, 4099


def look_at(position, target):
    """world-to-camera R (rows: right, down, forward) and T = -R position, float64"""
    forward = (target - position) / np.linalg.norm(target - position)
    right = np.cross(forward, np.array([0.0, -1.0, 0.0]))
    right /= np.linalg.norm(right)
    down = np.cross(forward, right)
    R = np.stack([right, down, forward])
    return R, -R @ position


def cameras():
    out = []
    for i in range(12):
        if i < 10:
            a = 2 * np.pi * i / 10
            position, target = np.array([3 * np.cos(a), 0.4, 3 * np.sin(a)]), np.zeros(3)
        elif i == 10:
            position, target = np.array([0.3, 0.1, -0.2]), np.array([2.0, 0.2, -0.1])
        else:
            position, target = np.array([-0.5, 0.2, 0.4]), np.array([-0.4, 0.1, -2.0])
        R, T = look_at(position, target)
        w, h = ((640, 480), (800, 600))[i % 2]
        fx = 500.0 + 20.0 * i
        out.append(types.SimpleNamespace(R=torch.tensor(R, dtype=torch.float32), T=torch.tensor(T, dtype=torch.float32),
                                         fx=torch.tensor(fx, dtype=torch.float32), fy=torch.tensor(fx + 7.0, dtype=torch.float32),
                                         width=torch.tensor(w, dtype=torch.int32), height=torch.tensor(h, dtype=torch.int32)))
    return out


class Observe(torch.overrides.TorchFunctionMode):
    def __init__(self):
        super().__init__()
        self.assigned, self.ors = [], []

    def __torch_function__(self, func, types_, args=(), kwargs=None):
        result = func(*args, **(kwargs or {}))
        if func is torch.Tensor.__setitem__:
            self.assigned.append(args[0].clone())
        elif func is torch.logical_or:
            self.ors.append(result)
        return result


def main(reference):
    for p in (reference, os.path.join(ROOT, "tests"), ROOT):
        sys.path.insert(0, p)
    import lightning_standin
    lightning_standin.install()
    import gspl_amd  # noqa: F401
    from gspl_amd import renderers  # noqa: F401   (the stand-ins of the native packages the reference imports)
    from internal.models.mip_splatting import MipSplattingUtils

    g = torch.Generator().manual_seed(20252)
    means = torch.rand(N_SEEN, 3, generator=g) * 3 - 1.5
    hidden = torch.rand(N_HIDDEN, 3, generator=g) * 3 - 1.5
    hidden[:, 1] = 60 + 10 * torch.rand(N_HIDDEN, generator=g)
    means = torch.cat([means, hidden])
    cams = cameras()
    table = torch.stack([torch.cat([c.R.reshape(9), c.T, torch.stack([c.fx, c.fy, c.width.float(), c.height.float()])]) for c in cams])

    with Observe() as seen:
        filt = MipSplattingUtils.compute_3d_filter(cams, types.SimpleNamespace(get_xyz=means))
    assert len(seen.assigned) == len(cams) + 1 and len(seen.ors) == len(cams)
    distance, valid_any = seen.assigned[-2], seen.ors[-1]
    assert tuple(filt.shape) == (N_SEEN + N_HIDDEN, 1) and not bool(valid_any[N_SEEN:].any())
    print(f"valid rows {int(valid_any.sum())} of {valid_any.numel()}; filter {float(filt.min()):.3e} .. {float(filt.max()):.3e}")
    out = {"means": means, "table": table, "filter": filt.detach(), "distance": distance, "valid_any": valid_any}

    a_scales = torch.exp(torch.randn(N_APPLY, 3, generator=g) - 4)
    a_opacities = torch.sigmoid(2 * torch.randn(N_APPLY, 1, generator=g))
    a_filter = 0.001 + 0.05 * torch.rand(N_APPLY, 1, generator=g)
    a_vs, a_vo = torch.randn(N_APPLY, 3, generator=g), torch.randn(N_APPLY, generator=g)
    out.update({"a_scales": a_scales, "a_opacities": a_opacities, "a_filter": a_filter, "a_vs": a_vs, "a_vo": a_vo})
    for comp in (False, True):
        s, o = a_scales.clone().requires_grad_(True), a_opacities.clone().requires_grad_(True)
        new_o, new_s = MipSplattingUtils.apply_3d_filter(filter_3d=a_filter, opacities=o, scales=s, opacity_compensation=comp)
        ((new_s * a_vs).sum() + (new_o[:, 0] * a_vo).sum()).backward()
        k = f"on{int(comp)}_"
        out.update({k + "opacities": new_o.detach(), k + "scales": new_s.detach(), k + "g_scales": s.grad, k + "g_opacities": o.grad})
    s = a_scales.clone().requires_grad_(True)
    new_s, coef = MipSplattingUtils.apply_3d_filter_on_scales(a_filter, s, True)
    ((new_s * a_vs).sum() + (coef * a_vo).sum()).backward()
    out.update({"sc_scales": new_s.detach(), "sc_coef": coef.detach(), "sc_g_scales": s.grad})
    assert MipSplattingUtils.apply_3d_filter_on_scales(a_filter, a_scales, False)[1] is None

    path = os.path.join(HERE, "ref_mip.npz")
    np.savez_compressed(path, **{k: v.numpy() for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])

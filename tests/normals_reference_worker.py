"""Worker of tests/test_normals_shims.py (its own process: the `lightning` / `torchmetrics` stand-ins must not leak into the other tests'
imports).

Imports the reference's OWN `internal.metrics.normal_reg` (unedited; its first statement is `from gsplat.utils import depth_to_normal`)
against the `gsplat` stand-in of `gspl_amd.compat`, and `internal.metrics.gs2d_metrics` next to `gspl_amd.surface.HipGS2DMetrics`, with
`ops.depth_to_normal` and `ops.surface_reg` bound — in this process only — to the fp64 oracle of tests/normals_oracle.py.  Prints one
JSON line.
usage: python normals_reference_worker.py <reference root>"""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_ROOT = sys.argv[1]
for p in (REF_ROOT, HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import lightning_standin  # noqa: E402
import normals_oracle as NO  # noqa: E402

lightning_standin.install()

import gspl_amd  # noqa: E402,F401
from gspl_amd import compat, ops  # noqa: E402

compat.install()
import gsplat  # noqa: E402

out = {"stand_in": "gspl_amd" in (gsplat.__doc__ or "")}
calls = []


def oracle_depth_to_normal(depth, rays, normalize_rays=False, channels_first=False):
    calls.append((tuple(depth.shape), bool(normalize_rays)))
    return NO.depth_to_normal(depth, rays, normalize_rays, channels_first)


ops.depth_to_normal = oracle_depth_to_normal
ops.surface_reg = lambda a, b, dist=None: NO.surface_reg(a, b, None if dist is None else dist.reshape(a.shape[1:]))

import internal.metrics.normal_reg as normal_reg  # noqa: E402
from gsplat.utils import depth_to_normal  # noqa: E402

out["normal_reg_uses_the_stand_in"] = normal_reg.depth_to_normal is depth_to_normal

# ---- get_normal_reg_metrics against the value computed by hand ------------------------------------------------------------------
H, W, seed = 37, 50, 3
g = torch.Generator().manual_seed(seed)
depth = NO.case_depth(H, W, seed).double()
R = NO.case_rotation(seed)
w2c = torch.eye(4, dtype=torch.float64)
w2c[:3, :3] = R.T
w2c[:3, 3] = torch.tensor([0.1, -0.2, 0.3], dtype=torch.float64)
K = torch.tensor([[170.0, 0, W / 2], [0, 168.0, H / 2], [0, 0, 1]], dtype=torch.float64)
alpha = torch.rand(1, H, W, generator=g, dtype=torch.float64)
normal = torch.randn(3, H, W, generator=g, dtype=torch.float64)
scales = torch.rand(40, 3, generator=g, dtype=torch.float64)
outputs = {"exp_depth": depth[None], "preprocessed_camera": (w2c[None], K[None], (W, H)), "alpha": alpha, "normal": normal}
me = types.SimpleNamespace(config=types.SimpleNamespace(normal_reg_lambda=0.05, flatten_reg=0.02))
model = types.SimpleNamespace(get_scales=lambda: scales)
metrics, pbar = {"loss": torch.zeros((), dtype=torch.float64)}, {}
normal_reg.NormalRegModuleMixin.get_normal_reg_metrics(me, model, outputs, None, metrics, pbar)
c2w = torch.linalg.inv(w2c)
A = c2w[:3, :3] @ torch.tensor([[1 / 170.0, 0, (0.5 - W / 2) / 170.0], [0, 1 / 168.0, (0.5 - H / 2) / 168.0], [0, 0, 1]], dtype=torch.float64)
n = NO.depth_to_normal(depth, A).permute(2, 0, 1) * alpha[0]
expect = 0.05 * (1 - (normal * n).sum(0)).mean() + 0.02 * scales[:, 2].mean()
out["normal_reg_loss"] = float(metrics["loss"])
out["normal_reg_expected"] = float(expect)
out["normal_reg_entries"] = sorted(metrics) + sorted(pbar)
out["depth_to_normal_calls"] = calls

# ---- HipGS2DMetrics next to the reference's GS2DMetrics -------------------------------------------------------------------------
import internal.metrics.gs2d_metrics as gs2d  # noqa: E402
from gspl_amd import surface  # noqa: E402

out["subclass"] = issubclass(surface.HipGS2DMetrics, gs2d.GS2DMetrics) and issubclass(surface.HipGS2DMetricsImpl, gs2d.GS2DMetricsImpl)
cfg = surface.HipGS2DMetrics(lambda_normal=0.05, lambda_dist=100.0)
out["fields"] = [cfg.lambda_normal, cfg.lambda_dist, gs2d.GS2DMetrics().lambda_normal, gs2d.GS2DMetrics().lambda_dist]
outs = {"rend_dist": torch.rand(1, H, W, generator=g, dtype=torch.float64), "rend_normal": normal, "surf_normal": n}
rows = []
for step in (100, 5000, 9000):
    pair = []
    for fn in (gs2d.GS2DMetricsImpl.train_metrics, surface.HipGS2DMetricsImpl.train_metrics):
        m, p = fn(types.SimpleNamespace(config=cfg), None, step, None, outs, ({"loss": torch.ones((), dtype=torch.float64)}, {}))
        pair.append([float(m["loss"]), float(m["normal_loss"]), float(m["dist_loss"]), sorted(p)])
    rows.append(pair)
out["gs2d"] = rows
print(json.dumps(out))

"""Worker of tests/test_spotless_shims.py (its own process: the `lightning` / `torchmetrics` stand-ins must not leak into the other
tests' imports).

Runs the reference's OWN, unedited `SpotLessMetricsModule` (internal/metrics/spotless_metrics.py) beside
`gspl_amd.spotless.HipSpotLessMetricsImpl` for three training steps on a 13 x 11 frame, on the CPU, with `ops.spotless_mask`,
`ops.spotless_error_stats` and `ops.spotless_masked_l1` bound — in this process only — to the fp64 oracle of tests/spotless_oracle.py.
Both modules see the same frames, the same weights and the same random draws.  Prints one JSON line.
usage: python spotless_reference_worker.py <reference root>"""
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lightning_standin  # noqa: E402
import spotless_oracle as SO  # noqa: E402

lightning_standin.install()

import gspl_amd  # noqa: E402,F401
from gspl_amd import ops  # noqa: E402


def _matrix(I, O):
    return torch.from_numpy(SO.resample_matrix(I, O))


def oracle_mask(G, A, B, w2, b2, out_size=None):
    """The oracle's forward in differentiable float64 torch ops (the float32 weights of SO.resample_matrix), returned as float32."""
    G, A, B, w2, b2 = (t.double() for t in (G, A, B, w2, b2))
    Ry, Rx = _matrix(G.shape[0], A.shape[0]), _matrix(G.shape[1], B.shape[0])
    z = torch.einsum("iy,jx,yxc->ijc", Ry, Rx, G) + A[:, None, :] + B[None, :, :]
    s = torch.sigmoid(torch.relu(z) @ w2.reshape(-1) + b2)
    if out_size is not None and tuple(out_size) != tuple(s.shape):
        s = _matrix(s.shape[0], out_size[0]) @ s @ _matrix(s.shape[1], out_size[1]).T
    return s.float()


def oracle_error_stats(render, gt, thresholds, bins, out=None):
    err = SO.error_map(render.detach().numpy(), gt.detach().numpy()).astype(np.float32)
    lower, upper = (np.float32(t) for t in thresholds.detach().numpy())
    return (torch.from_numpy(err), torch.from_numpy(SO.histogram(err, bins)).to(torch.int32), torch.from_numpy(SO.robust_mask(err, lower)),
            torch.from_numpy(SO.robust_mask(err, upper)))


def oracle_masked_l1(render, gt, mask):
    return (mask.detach().double().reshape(1, *render.shape[1:]) * (render.double() - gt.detach().double()).abs()).mean().float()


ops.spotless_mask, ops.spotless_error_stats, ops.spotless_masked_l1 = oracle_mask, oracle_error_stats, oracle_masked_l1

import internal.metrics.spotless_metrics as reference  # noqa: E402
from gspl_amd import spotless  # noqa: E402

out = {"subclass": issubclass(spotless.HipSpotLessMetrics, reference.SpotLessMetrics)
       and issubclass(spotless.HipSpotLessMetricsImpl, reference.SpotLessMetricsModule)}
fields = lambda cfg: {k: v for k, v in vars(cfg).items()}      # noqa: E731
out["same_fields_and_defaults"] = fields(spotless.HipSpotLessMetrics()) == fields(reference.SpotLessMetrics())

C, H0, W0, H, W = 24, 5, 7, 13, 11


class PlModule:
    """What the metric's hooks touch of the LightningModule."""
    batch_size = 1

    def __init__(self):
        self.on_after_backward_hooks, self.logged = [], {}

    def manual_backward(self, loss):
        loss.backward()

    def log(self, name, value, **kwargs):
        self.logged[name] = float(value.detach())


def build(config_class, size):
    cfg = config_class(n_feature_dims=C, bin_size=50, max_mlp_mask_size=size)
    module, pl = cfg.instantiate(), PlModule()
    module.setup("fit", pl)
    optimizers, _ = module.training_setup(pl)
    return module, pl, optimizers


def tensors(d):
    return {k: (v.detach().double().reshape(-1).tolist(), list(v.shape)) for k, v in d.items() if isinstance(v, torch.Tensor)}


runs = []
for size in (800, 9):
    g = torch.Generator().manual_seed(11 + size)
    theirs, their_pl, their_opt = build(reference.SpotLessMetrics, size)
    ours, our_pl, our_opt = build(spotless.HipSpotLessMetrics, size)
    run = {"size": size, "impl": type(ours).__name__, "hooks": [[h.__name__ for h in pl.on_after_backward_hooks] for pl in (their_pl, our_pl)],
           "optimizers": [len(their_opt), len(our_opt)],
           "state_names": [{k: list(v.shape) for k, v in m.state_dict().items()} for m in (theirs, ours)]}
    ours.load_state_dict(theirs.state_dict(), strict=True)            # each class loads the other's state dict strictly
    sf = torch.randn(C, H0, W0, generator=g)
    steps = []
    for k, step in enumerate((0, 500, 3000)):
        gt = torch.rand(3, H, W, generator=g)
        noise = (0.1 + 0.15 * k) * torch.randn(3, H, W, generator=g) * (torch.rand(1, H, W, generator=g) > 0.4)
        masked_pixels = (torch.rand(3, H, W, generator=g) > 0.8) if k == 2 else None      # the last step: the hook sees another ground truth
        row = {"step": step}
        for name, module, pl in (("theirs", theirs, their_pl), ("ours", ours, our_pl)):
            render = (gt + noise).clamp(0, 1).requires_grad_(True)
            outputs, batch = {"render": render}, (None, ("frame", gt.clone(), masked_pixels), sf)
            torch.manual_seed(1000 + step)                                                # the same bernoulli draws
            module.spotless_module.zero_grad()
            metrics, prog_bar = module.get_train_metrics(pl, None, step, batch, outputs)
            metrics["loss"].backward()
            for hook in pl.on_after_backward_hooks:
                hook(outputs, batch, None, step, pl)
            row[name] = {"metrics": {k_: float(v) for k_, v in metrics.items()}, "prog_bar": prog_bar, "logged": dict(pl.logged),
                         "outputs": tensors({k_: v for k_, v in outputs.items() if not k_.startswith("_")}),
                         "render_grad": render.grad.double().reshape(-1).tolist(),
                         "state": tensors(module.state_dict()),
                         "grads": tensors({n: p.grad for n, p in module.spotless_module.named_parameters()})}
        steps.append(row)
    run["steps"] = steps
    theirs.load_state_dict(ours.state_dict(), strict=True)
    runs.append(run)
out["runs"] = runs
print(json.dumps(out))

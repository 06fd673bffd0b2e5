"""Worker of tests/test_taming_shims.py (its own process: the `lightning` stand-in and the test-only `torchvision.transforms` must not
leak into the other tests' imports).

Imports the reference's OWN `Taming3DGSDensityControllerModule` (internal/density_controllers/taming_3dgs_density_controller.py,
unedited) and runs one densification event on a seeded CPU model next to `gspl_amd.taming.HipTaming3DGSDensityControllerImpl`:
`_densify_and_prune_with_scores`, then `_opacity_culling` with `densify_iter_num` below `cull_opacity_until`, with a GIVEN score vector.
The event runs three times from the same state and seed: the reference, the plugin (optimizer surgery through the reference's `Utils`,
which the plugin inherits with its base class), and the plugin with the stand-alone surgery of `gspl_amd.optim_utils` in `Utils`' place.
Then two events that must return early WITHOUT a random draw (a budget <= 0; all scores zero), each followed by one `torch.rand`.
Prints one JSON line.   usage: python taming_reference_worker.py <reference root>"""
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

lightning_standin.install()
import gspl_amd  # noqa: E402,F401
from gspl_amd import renderers  # noqa: E402,F401   (installs the stand-ins of gspl_amd.compat: gsplat, fused_ssim)

tv, tt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")          # test-only: nothing here calls them
tt.ToPILImage = tt.ToTensor = None
tv.transforms = tt
sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tt

from internal.density_controllers.taming_3dgs_density_controller import Taming3DGSDensityController  # noqa: E402
import internal.density_controllers.vanilla_density_controller as vanilla  # noqa: E402
from gspl_amd import optim_utils, taming as plugin  # noqa: E402

assert plugin.INSIDE_REFERENCE and issubclass(plugin.HipTaming3DGSDensityControllerImpl, vanilla.VanillaDensityControllerImpl)
REFERENCE_UTILS = vanilla.Utils


class StandAloneUtils:
    """`gspl_amd.optim_utils`' own surgery under the names the base class calls."""
    cat_tensors_to_properties = staticmethod(optim_utils._cat_parameters)
    prune_properties = staticmethod(optim_utils._prune_parameters)
    replace_tensors_to_properties = staticmethod(optim_utils._swap_parameters)


class Model(torch.nn.Module):
    """The parts of the reference's vanilla model the controller touches (internal/models/gaussian.py, vanilla_gaussian.py)."""

    def __init__(self, tensors):
        super().__init__()
        self.gaussians = {k: torch.nn.Parameter(v.clone()) for k, v in tensors.items()}

    properties = property(lambda s: s.gaussians, lambda s, v: setattr(s, "gaussians", dict(v)))
    property_names = property(lambda s: list(s.gaussians.keys()))
    n_gaussians = property(lambda s: s.gaussians["means"].shape[0])

    def get_property(self, name):
        return self.gaussians[name]

    def get_means(self):
        return self.gaussians["means"]

    def get_opacities(self):
        return torch.sigmoid(self.gaussians["opacities"])

    def get_scales(self):
        return torch.exp(self.gaussians["scales"])

    def opacity_inverse_activation(self, o):
        return torch.log(o / (1 - o))

    def scale_inverse_activation(self, s):
        return torch.log(s)


N0 = 3000
EXTENT = 5.0


def state0():
    g = torch.Generator().manual_seed(11)
    t = {"means": torch.randn(N0, 3, generator=g), "shs_dc": torch.randn(N0, 1, 3, generator=g), "shs_rest": torch.randn(N0, 15, 3, generator=g),
         "opacities": torch.randn(N0, 1, generator=g) * 2, "scales": torch.randn(N0, 3, generator=g) * 0.7 - 3.6,
         "rotations": torch.randn(N0, 4, generator=g)}
    t["opacities"][::9] = -7.0                            # sigmoid < 0.005: candidates of the opacity culling
    t["scales"][5::50] = -12.0                            # max scale < 1e-4: must be pruned
    grads = torch.rand(N0, generator=g) * 4e-4            # half of them above densify_grad_threshold
    scores = torch.rand(N0, generator=g) * (torch.rand(N0, generator=g) < 0.9)
    return t, grads, scores


class Logger:
    def __init__(self):
        self.logged = {}

    def log_metrics(self, metrics, step):
        self.logged.update({k: int(v) for k, v in metrics.items()})


def run(kind, budget_at_1, zero_scores=False, opacity_correction=False):
    tensors, grads, scores = state0()
    if zero_scores:
        scores = torch.zeros_like(scores)
    model = Model(tensors)
    opts = [torch.optim.Adam([{"params": [model.gaussians["means"]], "name": "means"}], lr=1e-3),
            torch.optim.Adam([{"params": [model.gaussians[k]], "name": k} for k in ("shs_dc", "shs_rest", "opacities", "scales", "rotations")], lr=1e-3)]
    g = torch.Generator().manual_seed(3)
    for p in model.gaussians.values():
        p.grad = torch.randn(p.shape, generator=g)
    for o in opts:
        o.step()
    cfg = dict(budget=2, opacity_correction=opacity_correction)
    vanilla.Utils = StandAloneUtils if kind == "standalone-surgery" else REFERENCE_UTILS
    ctl = (Taming3DGSDensityController(**cfg) if kind == "reference" else plugin.HipTaming3DGSDensityController(**cfg)).instantiate()
    # what setup("fit") leaves, without a trainer
    ctl.register_buffer("_densify_iter_num", torch.tensor(1, dtype=torch.int), persistent=True)
    ctl.cameras_extent = ctl.prune_extent = EXTENT
    ctl.counts_array = [N0, budget_at_1, budget_at_1 + 500]
    ctl._init_state(N0, torch.device("cpu"))
    logger = Logger()
    ctl.avoid_state_dict = (types.SimpleNamespace(logger=logger, trainer=types.SimpleNamespace(global_step=600)),)
    assert ctl.densify_iter_num == 1 and ctl.densify_iter_num < ctl.config.cull_opacity_until

    drawn = []
    multinomial = torch.multinomial

    def recording(*a, **k):
        out = multinomial(*a, **k)
        drawn.append((out.clone(), str(a[0].device)))
        return out
    torch.multinomial = recording
    torch.manual_seed(2024)
    try:
        with torch.no_grad():
            ctl._densify_and_prune_with_scores(grads=grads, scores=scores, gaussian_model=model, optimizers=opts)
            after_densify = model.n_gaussians
            ctl._opacity_culling(scores, None, model, opts)
        next_draw = torch.rand(4)
    finally:
        torch.multinomial = multinomial
        vanilla.Utils = REFERENCE_UTILS
    moments = {grp["name"]: (o.state[grp["params"][0]]["exp_avg"], o.state[grp["params"][0]]["exp_avg_sq"]) for o in opts for grp in o.param_groups}
    assert all(grp["params"][0] is model.gaussians[grp["name"]] for o in opts for grp in o.param_groups)
    assert ctl.xyz_gradient_accum.shape[0] == ctl.denom.shape[0] == ctl.max_radii2D.shape[0] == model.n_gaussians
    return {"after_densify": after_densify, "n": model.n_gaussians, "drawn": drawn, "next_draw": next_draw, "pruned": logger.logged.get("density/pruned"),
            "params": {k: v.detach().clone() for k, v in model.gaussians.items()}, "moments": moments}


def compare(ref, other):
    return {
        "n": other["n"], "after_densify": other["after_densify"],
        "indices_equal": len(other["drawn"]) == len(ref["drawn"]) and all(torch.equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(other["drawn"], ref["drawn"])),
        "next_draw_equal": torch.equal(other["next_draw"], ref["next_draw"]),
        "params_equal": sorted(k for k in ref["params"] if torch.equal(ref["params"][k], other["params"][k])),
        "moments_equal": sorted(k for k in ref["moments"] if all(torch.equal(a, b) for a, b in zip(ref["moments"][k], other["moments"][k]))),
    }


KINDS = (("plugin", "plugin"), ("standalone", "standalone-surgery"))
out = {}
for scenario, kwargs in (("event", dict(budget_at_1=3400)), ("event_opacity_correction", dict(budget_at_1=3400, opacity_correction=True)),
                         ("no_budget", dict(budget_at_1=N0 - 10)), ("zero_scores", dict(budget_at_1=3400, zero_scores=True))):
    ref = run("reference", **kwargs)
    entry = {"n0": N0, "n": ref["n"], "after_densify": ref["after_densify"], "budget": kwargs["budget_at_1"], "pruned": ref["pruned"],
             "draws": [int(d[0].numel()) for d in ref["drawn"]], "draw_devices": [d[1] for d in ref["drawn"]],
             "property_names": sorted(ref["params"])}
    for name, kind in KINDS:
        entry[name] = compare(ref, run(kind, **kwargs))
    out[scenario] = entry
print(json.dumps(out))

"""Worker of tests/test_mcmc_shims.py (its own process: the `lightning` stand-in and the test-only `gsplat.relocation` must not leak into
the other tests' imports).

Imports the reference's OWN `MCMCDensityControllerImpl` (internal/density_controllers/mcmc_density_controller.py, unedited) with
`gsplat.relocation.compute_relocation` bound to the fp64 oracle of tests/mcmc_oracle.py, and runs one relocation + growth event on a
seeded CPU model next to `gspl_amd.mcmc.HipMCMCDensityControllerImpl` whose op is the same oracle.  The event runs three times from the
same state and seed: the reference, the plugin (optimizer surgery through the reference's `Utils`), and the plugin with the stand-alone
surgery of `gspl_amd.optim_utils`.  Prints one JSON line: the sampled indices and whether every parameter and Adam moment agrees.
usage: python mcmc_reference_worker.py <reference root>"""
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
import mcmc_oracle as MO  # noqa: E402

lightning_standin.install()


def oracle_relocation(opacities, scales, ratios, binoms):
    o, s, _ = MO.relocation(opacities.double().numpy(), scales.double().numpy(), ratios.numpy(), binoms.shape[0])
    return torch.tensor(o, dtype=torch.float32), torch.tensor(s, dtype=torch.float32)


relocation = types.ModuleType("gsplat.relocation")          # test-only: what the CUDA package would provide
relocation.compute_relocation = oracle_relocation
if "gsplat" not in sys.modules:
    sys.modules["gsplat"] = types.ModuleType("gsplat")
sys.modules["gsplat.relocation"] = relocation

from internal.density_controllers.mcmc_density_controller import MCMCDensityController  # noqa: E402
import gspl_amd  # noqa: E402,F401
from gspl_amd import mcmc as plugin  # noqa: E402
from gspl_amd import optim_utils  # noqa: E402


class Model(torch.nn.Module):
    """The parts of the reference's vanilla model the controller touches (internal/models/gaussian.py, vanilla_gaussian.py:345-358)."""

    def __init__(self, tensors):
        super().__init__()
        self.gaussians = {k: torch.nn.Parameter(v.clone()) for k, v in tensors.items()}

    properties = property(lambda s: s.gaussians, lambda s, v: setattr(s, "gaussians", dict(v)))
    n_gaussians = property(lambda s: s.gaussians["means"].shape[0])
    opacities = property(lambda s: s.gaussians["opacities"])
    scales = property(lambda s: s.gaussians["scales"])
    means = property(lambda s: s.gaussians["means"])

    def get_property(self, name):
        return self.gaussians[name]

    def get_opacities(self):
        return torch.sigmoid(self.gaussians["opacities"])

    def get_scales(self):
        return torch.exp(self.gaussians["scales"])

    def opacity_inverse_activation(self, o):
        return torch.log(o / (1 - o))

    def scale_inverse_activation(self, s):
        return torch.log(s)


def state0(n=3000):
    g = torch.Generator().manual_seed(11)
    t = {"means": torch.randn(n, 3, generator=g), "shs_dc": torch.randn(n, 1, 3, generator=g), "shs_rest": torch.randn(n, 15, 3, generator=g),
         "opacities": torch.randn(n, 1, generator=g) * 2, "scales": torch.randn(n, 3, generator=g) - 4,
         "rotations": torch.randn(n, 4, generator=g)}
    t["opacities"][::9] = -7.0                            # sigmoid < 0.005: dead
    return t


def run(kind):
    model = Model(state0())
    opts = [torch.optim.Adam([{"params": [model.gaussians["means"]], "name": "means"}], lr=1e-3),
            torch.optim.Adam([{"params": [model.gaussians[k]], "name": k} for k in ("shs_dc", "shs_rest", "opacities", "scales", "rotations")], lr=1e-3)]
    g = torch.Generator().manual_seed(3)
    for p in model.gaussians.values():
        p.grad = torch.randn(p.shape, generator=g)
    for o in opts:
        o.step()
    cfg = dict(cap_max=3300, densify_from_iter=0, densification_interval=1)
    if kind == "reference":
        ctl = MCMCDensityController(**cfg).instantiate()
    else:
        ctl = plugin.HipMCMCDensityController(**cfg).instantiate()
        plugin._ops.compute_relocation = oracle_relocation
    if kind == "standalone-surgery":
        optim_utils.replace_tensors_to_properties = optim_utils._swap_parameters
        optim_utils.cat_tensors_to_properties = optim_utils._cat_parameters

    class Module:
        device = torch.device("cpu")
        gaussian_model = model
        on_train_batch_end_hooks = []
    ctl.setup("validate", Module)
    sampled = []
    orig = ctl._sample_alives
    ctl._sample_alives = lambda *a, **k: sampled.append(orig(*a, **k)) or sampled[-1]
    torch.manual_seed(2024)
    n0 = model.n_gaussians
    with torch.no_grad():
        dead = (model.get_opacities() <= ctl.config.min_opacity).squeeze(-1)
        ctl.relocate_gs(model, opts, dead)
        ctl.add_new_gs(model, opts)
    moments = {grp["name"]: (o.state[grp["params"][0]]["exp_avg"], o.state[grp["params"][0]]["exp_avg_sq"]) for o in opts for grp in o.param_groups}
    assert all(grp["params"][0] is model.gaussians[grp["name"]] for o in opts for grp in o.param_groups)
    return {"n0": n0, "n": model.n_gaussians, "dead": int(dead.sum()), "sampled": [i for i, _ in sampled],
            "params": {k: v.detach().clone() for k, v in model.gaussians.items()}, "moments": moments}


ref = run("reference")
hip = run("plugin")
alone = run("standalone-surgery")
out = {"n0": ref["n0"], "n": ref["n"], "dead": ref["dead"], "n_sampled": [len(i) for i in ref["sampled"]]}
for name, other in (("plugin", hip), ("standalone", alone)):
    out[name] = {
        "n": other["n"],
        "indices_equal": len(other["sampled"]) == len(ref["sampled"]) and all(torch.equal(a, b) for a, b in zip(other["sampled"], ref["sampled"])),
        "params_equal": sorted(k for k in ref["params"] if torch.equal(ref["params"][k], other["params"][k])),
        "moments_equal": sorted(k for k in ref["moments"] if all(torch.equal(a, b) for a, b in zip(ref["moments"][k], other["moments"][k]))),
    }
# the rows the surgery touched have zeroed moments, the others kept theirs
touched = torch.zeros(ref["n"], dtype=torch.bool)
for i in ref["sampled"]:
    touched[i] = True
touched[ref["n0"]:] = True
m = ref["moments"]["means"][1]
out["touched_rows_zeroed"] = bool((m[touched] == 0).all())
out["other_rows_kept"] = bool((m[~touched] != 0).all())
out["property_names"] = sorted(ref["params"])
print(json.dumps(out))

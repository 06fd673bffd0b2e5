"""Worker of tests/test_mip.py (its own process: the `lightning` stand-in and the reference's `internal` package must not leak into the
other tests' imports).

With the stand-ins of gspl_amd.compat installed it imports the reference's unedited internal.models.mip_splatting,
internal.renderers.gsplat_mip_splatting_renderer_v2 and internal.renderers.gsplat_appearance_embedding_renderer, and on the CPU, from
seeded parameters:
  * compares the config fields of the reference's classes with this package's;
  * runs the reference's OWN `MipSplattingModel.get_3d_filtered_scales_and_opacities`, `MipSplattingRendererMixin.get_scales` /
    `get_opacities` and `GSplatAppearanceEmbeddingMipRendererModule.get_scales` next to `gspl_amd`'s, on the reference's model and on
    `HipMipSplattingModel`, values and gradients, bit for bit (`opacity_compensation` on and off, and a pre-activated model);
  * runs `training_setup` of `HipMipSplattingModel` on the cameras of tests/golden/ref_mip.npz (the vanilla model's own
    `training_setup`, which needs a trainer, replaced by a recorder) and compares the filter with the reference's `compute_3d_filter`;
  * loads the reference model's state dict strictly into `HipMipSplattingModel`, and back.
(The appearance-Mip `get_opacities` needs the appearance model's colour kernels: tests/test_mip_renderer_gpu.py.)
Prints one JSON line.   usage: python mip_reference_worker.py <reference root>"""
import dataclasses
import json
import os
import sys
import types
import typing

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_ROOT = sys.argv[1]
for p in (REF_ROOT, HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

if not hasattr(torch, "Any"):          # the reference annotates with `torch.Any`, which newer torch no longer carries
    torch.Any = typing.Any

import lightning_standin  # noqa: E402

lightning_standin.install()

import gspl_amd  # noqa: E402,F401
from gspl_amd import mip, ops, renderers  # noqa: E402   (renderers installs the stand-ins of gspl_amd.compat)

import internal.models.mip_splatting as their_model  # noqa: E402
import internal.models.vanilla_gaussian as vanilla  # noqa: E402
import internal.renderers.gsplat_mip_splatting_renderer_v2 as their_v2  # noqa: E402
import internal.renderers.gsplat_appearance_embedding_renderer as their_appearance  # noqa: E402

assert mip.INSIDE_REFERENCE and issubclass(mip.HipMipSplattingModel, their_model.MipSplattingModel)
N = 777


def fields(cls):
    return {f.name: (f.default if f.default is not dataclasses.MISSING else repr(f.default_factory())) for f in dataclasses.fields(cls)}


def model_of(config, seed=5, pre_activated=False):
    m = config.instantiate()
    m.setup_from_number(N)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.gaussians["scales"].copy_(torch.randn(N, 3, generator=g) - 4)
        m.gaussians["opacities"].copy_(2 * torch.randn(N, 1, generator=g))
        m.gaussians["filter_3d"].copy_(0.001 + 0.05 * torch.rand(N, 1, generator=g))
        m.gaussians["means"].copy_(torch.randn(N, 3, generator=g))
    if pre_activated:
        m.pre_activate_all_properties()
    return m


def run(fn, model):
    """fn(model) -> tensors; the gradients of a seeded weighted sum of them with respect to the stored scales and opacities follow"""
    for p in model.gaussians.values():
        p.grad = None
    outs = [t for t in fn(model) if t is not None]
    g = torch.Generator().manual_seed(9)
    grads = []
    if any(t.requires_grad for t in outs):
        sum((t * torch.randn(t.shape, generator=g)).sum() for t in outs if t.requires_grad).backward()
        grads = [model.gaussians[k].grad for k in ("scales", "opacities")]
    return [t.detach().clone() for t in outs] + [x.clone() for x in grads if x is not None]


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def main():
    out = {"fields": {
        "model": [fields(their_model.MipSplatting), fields(mip.HipMipSplatting)],
        "v2": [fields(their_v2.GSplatMipSplattingRendererV2), fields(renderers.HipGSplatMipSplattingRendererV2)],
        "appearance_mip": [fields(their_appearance.GSplatAppearanceEmbeddingMipRenderer), fields(renderers.HipGSplatAppearanceEmbeddingMipRenderer)]}}

    their_mixin, our_mixin = their_v2.MipSplattingRendererMixin, renderers.HipMipSplattingRendererMixin
    their_am, our_am = their_appearance.GSplatAppearanceEmbeddingMipRendererModule, renderers.HipGSplatAppearanceEmbeddingMipRendererModule
    checks, raw_flags = {}, {}
    for compensation in (True, False):
        for pre in (False, True):
            key = f"compensation={compensation},pre_activated={pre}"
            theirs = model_of(their_model.MipSplatting(opacity_compensation=compensation), pre_activated=pre)
            ours = model_of(mip.HipMipSplatting(opacity_compensation=compensation), pre_activated=pre)
            reference = {"model": run(lambda m: their_model.MipSplattingModel.get_3d_filtered_scales_and_opacities(m), theirs),
                         "mixin": run(lambda m: their_mixin.get_scales(None, None, m), theirs),
                         "appearance": run(lambda m: their_am.get_scales(None, None, m), theirs)}
            got = {}
            for name, model in (("reference model", theirs), ("hip model", ours)):
                got[name] = {"model": same(reference["model"], run(lambda m: mip.filtered_scales_and_opacities(m), model)),
                             "mixin": same(reference["mixin"], run(lambda m: our_mixin.get_scales(None, None, m), model)),
                             "appearance": same(reference["appearance"], run(lambda m: our_am.get_scales(None, None, m), model))}
            got["hip model"]["method"] = same(reference["model"], run(lambda m: m.get_3d_filtered_scales_and_opacities(), ours))
            got["n_outputs"] = {k: len(v) for k, v in reference.items()}
            checks[key] = got
            raw_flags[key] = [mip._stored_or_activated(theirs, "scales", "scale_activation", "get_scales")[1],
                              mip._stored_or_activated(ours, "opacities", "opacity_activation", "get_opacities")[1]]
    status = torch.randn(5)
    out["checks"], out["raw_flags"] = checks, raw_flags
    out["get_opacities"] = [their_mixin.get_opacities(None, None, None, None, None, status)[0] is status and their_mixin.get_opacities(None, None, None, None, None, status)[1] is None,
                            our_mixin.get_opacities(None, None, None, None, None, status)[0] is status and our_mixin.get_opacities(None, None, None, None, None, status)[1] is None]

    # training_setup: the table once, the filter by one op call
    with np.load(os.path.join(HERE, "golden", "ref_mip.npz")) as z:
        means, table, want = torch.from_numpy(z["means"]), torch.from_numpy(z["table"]), torch.from_numpy(z["filter"])
    cameras = [types.SimpleNamespace(R=r[:9].reshape(3, 3), T=r[9:12], fx=r[12], fy=r[13], width=r[14].to(torch.int32), height=r[15].to(torch.int32))
               for r in table]
    model = mip.HipMipSplatting().instantiate()
    model.setup_from_number(means.shape[0])
    with torch.no_grad():
        model.gaussians["means"].copy_(means)
    called = []
    vanilla.VanillaGaussianModel.training_setup = lambda self, module: called.append(module) or ("optimizers", "schedulers")
    calls, real = [], ops.mip_camera_table
    ops.mip_camera_table = lambda *a, **k: calls.append(1) or real(*a, **k)
    module = types.SimpleNamespace(trainer=types.SimpleNamespace(datamodule=types.SimpleNamespace(dataparser_outputs=types.SimpleNamespace(
        train_set=types.SimpleNamespace(cameras=cameras)))))
    returned = model.training_setup(module)
    first = model.get_3d_filter().clone()
    model.compute_3d_filter()
    theirs = their_model.MipSplattingUtils.compute_3d_filter(cameras, model)
    out["training_setup"] = {"returned": list(returned), "vanilla_called": called == [module], "tables_built": len(calls),
                             "table_equal": torch.equal(model._camera_table, table), "filter_is_golden": torch.equal(first, want),
                             "filter_is_reference": torch.equal(model.get_3d_filter(), theirs.detach()),
                             "is_parameter": isinstance(model.gaussians["filter_3d"], torch.nn.Parameter) and not model.gaussians["filter_3d"].requires_grad,
                             "names": list(model.get_property_names())}

    # checkpoints, both ways
    theirs, ours = model_of(their_model.MipSplatting(), seed=21), mip.HipMipSplatting().instantiate()
    ours.setup_from_number(N)
    there = ours.load_state_dict(theirs.state_dict(), strict=True)
    back = model_of(their_model.MipSplatting(), seed=22)
    here = back.load_state_dict(ours.state_dict(), strict=True)
    out["state_dict"] = {"keys_equal": list(theirs.state_dict()) == list(ours.state_dict()), "has_filter": "gaussians.filter_3d" in ours.state_dict(),
                         "loaded": not there.missing_keys and not there.unexpected_keys and not here.missing_keys and not here.unexpected_keys,
                         "values_equal": all(torch.equal(v, back.state_dict()[k]) and torch.equal(v, ours.state_dict()[k]) for k, v in theirs.state_dict().items())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

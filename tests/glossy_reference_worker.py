"""Worker of tests/test_glossy.py (its own process: the `lightning` stand-in and the reference's `internal` package must not leak into
the other tests' imports).

With the stand-ins of gspl_amd.compat installed it imports the reference's unedited internal.renderers.glossy_renderer, compares the
fields of its `GlossyRenderer` with `gspl_amd.renderers.HipGlossyRenderer`, and runs the reference's OWN
`GlossyGaussianModel.get_view_dep_opacities` + clamp in float64 on the inputs of tests/golden/ref_glossy.npz.  Prints one JSON line.
usage: python glossy_reference_worker.py <reference root>"""
import dataclasses
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

lightning_standin.install()

import gspl_amd  # noqa: E402,F401
from gspl_amd import renderers  # noqa: E402   (installs the stand-ins of gspl_amd.compat)

import internal.renderers.glossy_renderer as theirs  # noqa: E402
from internal.models.glossy_gaussian import GlossyGaussianModel  # noqa: E402


def fields(cls):
    return {f.name: f.default for f in dataclasses.fields(cls)}


def main():
    with np.load(os.path.join(HERE, "golden", "ref_glossy.npz")) as z:
        ref = {k: torch.from_numpy(z[k]) for k in ("means", "camera", "dc", "rest")}
    values = []
    for degree in range(5):
        model = types.SimpleNamespace(active_sh_degree=degree, _opacity_name="opacities", _opacity_rest_name="opacity_rest",
                                      properties={"opacities": ref["dc"], "opacity_rest": ref["rest"]})
        d = torch.nn.functional.normalize(ref["means"] - ref["camera"], dim=-1)
        raw = GlossyGaussianModel.get_view_dep_opacities(model, dirs=d, masks=None).squeeze(-1)
        values.append(torch.clamp(raw, min=0., max=1.).tolist())
    print(json.dumps({"imported": theirs.GlossyRenderer.__module__, "their_fields": fields(theirs.GlossyRenderer),
                      "our_fields": fields(renderers.HipGlossyRenderer),
                      "module_is_v1": issubclass(theirs.GlossyRendererModule, theirs.GSplatV1RendererModule), "values": values}))


if __name__ == "__main__":
    main()

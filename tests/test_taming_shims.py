"""The Taming-3DGS plugin next to the reference's own controller, without a GPU (skipped where the reference tree is absent, as
tests/test_mcmc_shims.py is): the configuration's fields and defaults, and one densification event — `_densify_and_prune_with_scores`,
then `_opacity_culling` — of the reference's unedited `Taming3DGSDensityControllerModule`, of `gspl_amd.taming`'s controller, and of the
latter with `gspl_amd.optim_utils`' surgery, from one seeded state, one seed and one given score vector
(tests/taming_reference_worker.py, in a process of its own)."""
import ast
import dataclasses
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = os.environ.get("GSPL_REFERENCE_ROOT", "/root/reference")
REF_CONTROLLER = os.path.join(REF_ROOT, "internal", "density_controllers", "taming_3dgs_density_controller.py")
needs_reference = pytest.mark.skipif(not os.path.exists(REF_CONTROLLER), reason="reference tree not present")


def _reference_fields(class_name):
    tree = ast.parse(open(REF_CONTROLLER).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == class_name)
    out = {}
    for st in cls.body:
        if isinstance(st, ast.AnnAssign) and isinstance(st.target, ast.Name):
            try:
                out[st.target.id] = ast.literal_eval(st.value) if st.value is not None else dataclasses.MISSING
            except ValueError:
                out[st.target.id] = ast.unparse(st.value)          # `ScoreCoefficients()`
    return out


@needs_reference
def test_plugin_fields_and_defaults_equal_the_reference():
    import gspl_amd  # noqa: F401
    from gspl_amd.taming import HipTaming3DGSDensityController, ScoreCoefficients
    ref = _reference_fields("Taming3DGSDensityController")
    ours = {f.name: (f.default if f.default is not dataclasses.MISSING else f.default_factory()) for f in dataclasses.fields(HipTaming3DGSDensityController)}
    assert ours.pop("edges_on_cpu") is False                      # this package's one addition, last
    assert list(ours)[:len(ref)] == list(ref)
    assert ref.pop("score_coeffs") == "ScoreCoefficients()" and ours.pop("score_coeffs") == ScoreCoefficients()
    assert ours == ref
    coeffs = _reference_fields("ScoreCoefficients")
    assert {f.name: f.default for f in dataclasses.fields(ScoreCoefficients)} == coeffs and list(coeffs)[0] == "view_importance"


@pytest.fixture(scope="module")
def events():
    r = subprocess.run([sys.executable, os.path.join(HERE, "taming_reference_worker.py"), REF_ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def _same(entry):
    for variant in ("plugin", "standalone"):
        v = entry[variant]
        assert v["n"] == entry["n"] and v["after_densify"] == entry["after_densify"], variant
        assert v["indices_equal"] and v["next_draw_equal"], variant
        assert v["params_equal"] == entry["property_names"] and v["moments_equal"] == entry["property_names"], variant


@needs_reference
@pytest.mark.parametrize("scenario", ["event", "event_opacity_correction"])
def test_reference_controller_and_plugin_densify_identically(events, scenario):
    d = events[scenario]
    # three draws: clones and splits on the scores' device, the culling's on the CPU; clones + splits fill the budget curve's step
    assert len(d["draws"]) == 3 and all(n > 0 for n in d["draws"]) and d["draw_devices"][2] == "cpu"
    assert d["after_densify"] == d["n0"] + d["draws"][0] + d["draws"][1] <= d["budget"]          # a split adds 2 and removes 1
    assert d["n"] == d["after_densify"] - d["pruned"] < d["after_densify"] and d["n"] <= d["budget"]
    _same(d)


@needs_reference
@pytest.mark.parametrize("scenario", ["no_budget", "zero_scores"])
def test_early_returns_draw_nothing(events, scenario):
    """A budget <= 0 (the curve below the current count) and scores that sum to zero leave clone and split without a draw: the only
    multinomial is the culling's, and the next draw of the global generator is the same on all three."""
    d = events[scenario]
    assert d["after_densify"] == d["n0"] and len(d["draws"]) == 1 and d["draw_devices"] == ["cpu"]
    assert d["n"] == d["n0"] - d["pruned"]
    _same(d)

"""The Glossy-Gaussian route without a GPU: the fp64 oracle tests/glossy_oracle.py against the reference's own float64 run
(tests/golden/ref_glossy.npz, made by tests/golden/make_glossy_golden.py from `eval_sh_decomposed`), the reference's unedited model
method next to it (tests/glossy_reference_worker.py, a process of its own; skipped without the reference tree), the plugin's config and
every refusal of `ops.sh_view_opacities` that needs no device."""
import dataclasses
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import glossy_oracle as GO

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_glossy.npz")
REF_ROOT = os.environ.get("GSPL_REFERENCE_ROOT", "/root/reference")
needs_reference = pytest.mark.skipif(not os.path.exists(os.path.join(REF_ROOT, "internal", "renderers", "glossy_renderer.py")),
                                     reason="the reference tree is not present")
FRAGILE_CAP = 1e-3          # of the rows may lie within the float32 bound of a threshold (tests/test_glossy_gpu.py counts the bound)


@pytest.fixture(scope="module")
def ref():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def worker():
    r = subprocess.run([sys.executable, os.path.join(HERE, "glossy_reference_worker.py"), REF_ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("degree", range(5))
def test_oracle_matches_the_reference_run(ref, degree):
    """Values and gradients within 1e-12: the project's standing figure for an fp64 oracle against the reference's float64 run."""
    o = GO.opacity(degree, ref["means"], ref["camera"], ref["dc"], ref["rest"], ref["w"])
    for name, got, want in (("raw", o["raw"], ref[f"raw{degree}"]), ("value", o["value"], ref[f"value{degree}"]),
                            ("v_dc", o["v_dc"], ref[f"v_dc{degree}"].reshape(-1)), ("v_rest", o["v_rest"], ref[f"v_rest{degree}"][..., 0])):
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12, f"degree {degree}: {name}"
    K = (degree + 1) ** 2
    assert not o["v_rest"][:, K - 1:].any() and (degree == 0 or o["v_rest"][:, :K - 1].any())


@pytest.mark.parametrize("degree", range(5))
def test_the_fixture_covers_the_three_regimes_and_the_zero_direction(ref, degree):
    """At least 10 % of the rows below 0, inside and above 1 at every degree; row 7 sits at the camera: d = 0, finite, interior, and at
    degree 4 the constant 3 C4[4] of its one non-zero basis polynomial shows."""
    raw = ref[f"raw{degree}"]
    shares = np.array([(raw < 0).mean(), ((raw >= 0) & (raw <= 1)).mean(), (raw > 1).mean()])
    assert shares.min() >= 0.10, shares
    assert np.array_equal(ref["means"][7], ref["camera"]) and ref["dc"][7, 0, 0] == 0.0
    assert not GO.directions(ref["means"], ref["camera"])[7].any() and np.isfinite(raw).all() and 0.0 < raw[7] < 1.0
    expected = 0.5 + (3 * GO.C4[4] * ref["rest"][7, 19, 0] if degree == 4 else 0.0)
    assert abs(raw[7] - expected) <= 1e-15 and (degree < 4 or abs(raw[7] - 0.5) > 1e-3)


@pytest.mark.parametrize("degree", range(5))
def test_near_threshold_rows_are_rare(ref, degree):
    """Rows whose float64 value lies within the kernel's float32 bound of 0 or 1 may take either branch of the clamp's gradient; they
    are at most 1e-3 of the rows (the GPU tests assert the same cap on their own cases)."""
    from test_glossy_gpu import value_bound
    o = GO.opacity(degree, ref["means"], ref["camera"], ref["dc"], ref["rest"])
    bound = value_bound(degree, o, ref["rest"][..., 0])
    near = (np.abs(o["raw"]) <= bound) | (np.abs(o["raw"] - 1.0) <= bound)
    print(f"degree {degree}: {int(near.sum())} of {near.size} rows within the bound of a threshold (largest bound {bound.max():.3e})")
    assert near.mean() <= FRAGILE_CAP


@needs_reference
def test_the_reference_model_method_matches_the_oracle(worker, ref):
    """`GlossyGaussianModel.get_view_dep_opacities` + clamp, unedited, in float64."""
    for degree in range(5):
        o = GO.opacity(degree, ref["means"], ref["camera"], ref["dc"], ref["rest"])
        assert np.abs(np.asarray(worker["values"][degree]) - o["value"]).max() <= 1e-12, degree


@needs_reference
def test_the_reference_renderer_imports_with_the_stand_ins(worker):
    assert worker["imported"] == "internal.renderers.glossy_renderer" and worker["module_is_v1"]
    theirs, ours = worker["their_fields"], worker["our_fields"]
    # (separate_sh: this package's gsplat-v1 plugin reads shs_dc / shs_rest in place by default, the reference concatenates them)
    assert sorted(theirs) == sorted(ours) and all(ours[k] == theirs[k] for k in theirs if k != "separate_sh"), (theirs, ours)


def test_config_instantiates_with_the_v1_fields():
    from gspl_amd import renderers
    v1 = {f.name: f.default for f in dataclasses.fields(renderers.HipGSplatV1Renderer)}
    assert {f.name: f.default for f in dataclasses.fields(renderers.HipGlossyRenderer)} == v1
    cfg = renderers.HipGlossyRenderer(block_size=16, anti_aliased=False, filter_2d_kernel_size=0.1, separate_sh=True, tile_based_culling=False,
                                      max_viewspace_grad_scale=100.)
    module = cfg.instantiate()
    assert isinstance(module, renderers.HipGlossyRendererModule) and isinstance(module, renderers.HipGSplatV1RendererModule)
    assert module.config is cfg and type(module).get_rgbs is renderers.HipGSplatV1RendererModule.get_rgbs
    overridden = [n for n, v in vars(renderers.HipGlossyRendererModule).items() if callable(v)]
    assert overridden == ["get_opacities"]


def test_a_model_without_opacity_rest_is_refused():
    from gspl_amd import renderers
    module = renderers.HipGlossyRenderer().instantiate()
    model = types.SimpleNamespace(properties={"opacities": torch.zeros(4, 1)}, active_sh_degree=0, get_xyz=torch.zeros(4, 3))
    with pytest.raises(TypeError, match="GlossyGaussian"):
        module.get_opacities(types.SimpleNamespace(camera_center=torch.zeros(3)), model, None, None, None)


def _inputs(N=5, Kr=15, dtype=torch.float32):
    return torch.zeros(N, 3, dtype=dtype), torch.zeros(3, dtype=dtype), torch.zeros(N, 1, 1, dtype=dtype), torch.zeros(N, Kr, 1, dtype=dtype)


@pytest.mark.parametrize("entry", ["sh_view_opacities", "sh_view_opacities_forward"])
def test_refusals(entry):
    from gspl_amd import ops
    fn = getattr(ops, entry)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(3, *_inputs())
    with pytest.raises(NotImplementedError, match="float32"):
        fn(3, *_inputs(dtype=torch.float64))
    means, camera, dc, rest = _inputs()
    with pytest.raises(NotImplementedError, match="float32"):
        fn(3, means, camera, dc.half(), rest)
    for degree in (-1, 5):
        with pytest.raises(ValueError, match=rf"degree must be 0 \.\. 4, got {degree} .*15 columns"):
            fn(degree, *_inputs())
    with pytest.raises(ValueError, match="degree 3 needs 15 columns of opacity_rest, got 8"):
        fn(3, *_inputs(Kr=8))
    with pytest.raises(ValueError, match="degree 1 needs 3 columns of opacity_rest, got 0"):
        fn(1, *_inputs(Kr=0))
    with pytest.raises(ValueError, match="opacity_dc"):
        fn(3, means, camera, dc.reshape(1, 5), rest)
    with pytest.raises(ValueError, match="opacity_rest"):
        fn(3, means, camera, dc, torch.zeros(5, 15, 3))


def test_backward_launch_refusals():
    from gspl_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sh_view_opacities_backward(3, *_inputs(), torch.zeros(5))
    with pytest.raises(ValueError, match="degree 4 needs 24 columns of opacity_rest, got 15"):
        ops.sh_view_opacities_backward(4, *_inputs(), torch.zeros(5))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """The C entry points themselves (include/gspl_hip.h section 25): a degree outside 0 .. 4, too few or too many columns, a NULL
    required pointer and a `rest` pointer that does not go with n_rest return the library's invalid-argument code; N = 0 succeeds
    without a launch.  None of these calls reaches the device."""
    import ctypes
    from gspl_amd import _lib as L
    lib = L.lib()
    block = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(block))

    def fwd(N, degree, Kr, means=p, rest=p, out=p):
        return lib.gspl_sh_opacity_fwd(N, degree, Kr, means, p, p, rest, out, None)

    def bwd(N, degree, Kr, rest=p, v=p, v_dc=p, v_rest=p):
        return lib.gspl_sh_opacity_bwd(N, degree, Kr, p, p, p, rest, v, v_dc, v_rest, None)

    bad = L.GSPL_ERR_INVALID_ARG
    for call in (fwd, bwd):
        assert call(4, 5, 24) == bad and call(4, -1, 24) == bad and call(-1, 3, 15) == bad
        assert call(4, 3, 14) == bad and call(4, 4, 15) == bad and call(4, 1, 0, rest=None) == bad and call(4, 0, 62) == bad
        assert call(4, 3, 15, rest=None) == bad and call(4, 0, 0, rest=p) == bad
        assert b"sh_opacity" in lib.gspl_last_error()
        assert call(0, 3, 15) == L.GSPL_OK and call(0, 0, 0, rest=None, **({"v_rest": None} if call is bwd else {})) == L.GSPL_OK
    assert fwd(4, 3, 15, means=None) == bad and fwd(4, 3, 15, out=None) == bad
    assert bwd(4, 3, 15, v=None) == bad and bwd(4, 3, 15, v_dc=None) == bad and bwd(4, 3, 15, v_rest=None) == bad and bwd(4, 0, 0, rest=None) == bad

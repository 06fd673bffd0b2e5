"""The `diff_accel_gaussian_rasterization` stand-in (Taming 3DGS's rasterizer package, internal/renderers/taming_3dgs_renderer.py:4,
internal/optimizers.py:63-90): registered by `compat.install()`, driven by the reference's own `Taming3DGSRenderer` unedited.

CPU: the fused HIP call behind the stand-in (`ops.inria.rasterize_inria_accel`) is swapped — in this test — for the fp64 oracle of
tests/accel_oracle.py; what is checked is the wiring: module names, the dc / shs split, the `antialiasing` field, the triple return."""
import os
import sys

import pytest
import torch

from oracle import gsplat_oracle as O
import accel_oracle as A

REF_ROOT = os.environ.get("GSPL_REFERENCE_ROOT", "/root/reference")
needs_reference = pytest.mark.skipif(not os.path.exists(os.path.join(REF_ROOT, "internal", "renderers", "taming_3dgs_renderer.py")),
                                     reason="reference tree not present")


def _standin():
    import gspl_amd  # noqa: F401
    from gspl_amd import compat
    compat.install()
    import diff_accel_gaussian_rasterization as dagr
    if "gspl_amd" not in (dagr.__doc__ or ""):
        pytest.skip("a real diff_accel_gaussian_rasterization package is installed")
    return dagr


def test_accel_stand_in_exposes_the_three_names():
    dagr = _standin()
    from gspl_amd import ops, optimizers
    from diff_accel_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, SparseGaussianAdam
    assert GaussianRasterizer is ops.AccelGaussianRasterizer and GaussianRasterizationSettings is ops.AccelRasterizationSettings
    assert SparseGaussianAdam is optimizers.SparseGaussianAdam and issubclass(SparseGaussianAdam, torch.optim.Adam)
    assert "antialiasing" in GaussianRasterizationSettings._fields and GaussianRasterizationSettings._field_defaults["antialiasing"] is False
    # the vanilla stand-in keeps its own settings (no antialiasing field) and its 2-tuple rasterizer
    assert "antialiasing" not in ops.GaussianRasterizationSettings._fields
    assert dagr.GaussianRasterizer is not ops.GaussianRasterizer


def _oracle_accel(calls):
    def fake(settings, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None,
             shs_rest=None, raw_parameters=False, antialiasing=False, inverse_depth=True):
        assert not raw_parameters
        s = settings
        calls.append(dict(antialiasing=antialiasing, inverse_depth=inverse_depth, shs_rest=shs_rest is not None,
                          colors_precomp=colors_precomp is not None))
        sh = None if shs is None else (shs if shs_rest is None else torch.cat([shs, shs_rest], dim=1))
        r = A.render_inria_accel(means3D, scales, rotations, opacities, sh, s.sh_degree, s.viewmatrix, s.projmatrix, s.campos,
                                 s.tanfovx, s.tanfovy, s.image_width, s.image_height, s.bg, antialias=antialiasing,
                                 scale_modifier=s.scale_modifier, colors_precomp=colors_precomp)
        return r["render"], r["radii"], (r["inverse_depth"] if inverse_depth else None)
    return fake


def _ref(params, cam, bg, antialias, colors_precomp=None):
    return A.render_inria_accel(*params[:4], params[4], 3, cam["world_to_camera"].double(), cam["full_projection"].double(),
                                cam["camera_center"].double(), cam["tanfovx"], cam["tanfovy"], cam["width"], cam["height"], bg,
                                antialias=antialias, colors_precomp=colors_precomp)


@needs_reference
@pytest.mark.parametrize("anti_aliased", [False, True])
@pytest.mark.parametrize("form", ["shs", "colors_precomp", "pre_activated"])
def test_reference_taming_renderer_runs_unedited_on_the_stand_in(monkeypatch, anti_aliased, form):
    _standin()
    from test_package_shims import _stubs, _scene, _Cam
    _stubs()
    from fakes import FakeGaussianModel
    import gspl_amd.ops.inria as inria
    import internal.renderers.taming_3dgs_renderer as tr                         # imports from the stand-in
    import diff_accel_gaussian_rasterization as dagr
    assert tr.GaussianRasterizer is dagr.GaussianRasterizer and tr.GaussianRasterizationSettings is dagr.GaussianRasterizationSettings
    calls = []
    monkeypatch.setattr(inria, "rasterize_inria_accel", _oracle_accel(calls))
    params, cam, bg = _scene(seed=7)
    params = (params[0], params[1] * 0.6, *params[2:])          # smaller splats: some reach the 2.5e-5 floor sooner
    model = FakeGaussianModel(*[p.clone() for p in params])
    kwargs = {}
    cp = None
    if form == "colors_precomp":
        cp = torch.rand(params[0].shape[0], 3, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
        kwargs["colors_precomp"] = cp
    if form == "pre_activated":
        model.is_pre_activated = True
        model.get_shs = lambda: model.get_features
    renderer = tr.Taming3DGSRenderer(anti_aliased=anti_aliased).instantiate()
    out = renderer(_Cam(cam), model, bg, render_types=["rgb", "inverse_depth"], **kwargs)
    assert calls and calls[-1]["antialiasing"] is anti_aliased and calls[-1]["inverse_depth"] is True
    assert calls[-1]["colors_precomp"] is (form == "colors_precomp")
    assert calls[-1]["shs_rest"] is (form != "colors_precomp")          # dc / shs -> shs / shs_rest
    ref = _ref(params, cam, bg, anti_aliased, colors_precomp=cp)
    assert out["render"].shape == (3, cam["height"], cam["width"]) and out["inverse_depth"].shape == (1, cam["height"], cam["width"])
    assert float((out["render"] - ref["render"]).abs().max()) <= 1e-9
    assert float((out["inverse_depth"] - ref["inverse_depth"]).abs().max()) <= 1e-9
    assert torch.equal(out["radii"], ref["radii"]) and torch.equal(out["visibility_filter"], ref["radii"] > 0)
    assert float(out["inverse_depth"].max()) > 0.0
    outputs = renderer.get_available_outputs()
    assert set(outputs) == {"rgb", "inverse_depth"} and outputs["inverse_depth"].key == "inverse_depth"


def test_oracle_antialiasing_changes_the_image_and_floors_needles():
    """The oracle's compensation is the published rule: 1 > comp >= sqrt(2.5e-5), a needle-thin splat sits at the floor."""
    from test_package_shims import _scene
    params, cam, bg = _scene(seed=8)
    means, scales, quats = params[0], params[1].clone(), params[2]
    scales[:20, 1:] = 1e-7                                         # needles: det0 / det1 far below 2.5e-5
    comp = A.compensation(means, scales, 1.0, quats, cam["world_to_camera"].double(), cam["tanfovx"], cam["tanfovy"], cam["width"], cam["height"])
    front = A.view_depth(means, cam["world_to_camera"].double()) > 0.2
    assert bool((comp[front] <= 1.0).all()) and bool((comp[front] >= 2.5e-5 ** 0.5 - 1e-15).all())
    assert bool(torch.isclose(comp[:20][front[:20]], torch.tensor(2.5e-5 ** 0.5, dtype=torch.float64)).all())


@needs_reference
def test_reference_sparse_gaussian_adam_config_builds_the_stand_in():
    _standin()
    from test_package_shims import _stubs
    _stubs()
    import internal.optimizers as io
    from gspl_amd import optimizers
    p = torch.nn.Parameter(torch.zeros(8, 3))
    opt = io.SparseGaussianAdam().instantiate([{"params": [p], "name": "means"}], 1e-3, eps=1e-15)
    assert isinstance(opt, optimizers.SparseGaussianAdam) and isinstance(opt, torch.optim.Adam)
    assert opt.param_groups[0]["betas"] == (0.9, 0.999) and opt.param_groups[0]["eps"] == 1e-15 and opt.param_groups[0]["lr"] == 1e-3


def test_hip_optimizer_config_and_renderer_plugin():
    import pickle
    from gspl_amd import optimizers
    from gspl_amd.renderers import HipTaming3DGSRenderer
    p = torch.nn.Parameter(torch.zeros(8, 3))
    opt = optimizers.HipSparseGaussianAdam().instantiate([{"params": [p], "name": "means"}], 1e-3)
    assert isinstance(opt, optimizers.SparseGaussianAdam) and isinstance(opt, torch.optim.Adam)
    r = HipTaming3DGSRenderer(anti_aliased=True)
    r2 = pickle.loads(pickle.dumps(r))
    assert r2.anti_aliased and r2.filter_2d_kernel_size == 0.3
    assert set(r.get_available_outputs()) == {"rgb", "inverse_depth"}
    with pytest.raises(AssertionError):
        HipTaming3DGSRenderer(anti_aliased=True, filter_2d_kernel_size=0.1)


def test_staged_orchestration_refuses_the_new_switches():
    from gspl_amd import ops
    s = ops.AccelRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3))
    old = ops.FUSED_INRIA
    ops.FUSED_INRIA = False
    try:
        with pytest.raises(NotImplementedError):
            ops.rasterize_inria_accel(s, torch.zeros(1, 3), torch.zeros(1, 3), torch.ones(1, 1), colors_precomp=torch.zeros(1, 3),
                                      scales=torch.ones(1, 3), rotations=torch.tensor([[1.0, 0, 0, 0]]), antialiasing=True)
    finally:
        ops.FUSED_INRIA = old

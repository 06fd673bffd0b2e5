"""The `diff_surfel_rasterization` stand-in (2D Gaussian Splatting, internal/renderers/vanilla_2dgs_renderer.py:14): registered by
`compat.install()`, driven by the reference's own `Vanilla2DGSRenderer` unedited, and the `HipVanilla2DGSRenderer` plugin.

CPU: the HIP op behind the stand-in (`ops.surfel.rasterize_surfels`) is swapped — in this test — for the fp64 oracle of
tests/surfel_oracle.py; what is checked is the wiring (module names, argument lists, the triple return, the output dict).  The oracle
itself is pinned by closed forms."""
import math
import os

import pytest
import torch

from oracle import gsplat_oracle as O
import surfel_oracle as SO

REF_ROOT = os.environ.get("GSPL_REFERENCE_ROOT", "/root/reference")
needs_reference = pytest.mark.skipif(not os.path.exists(os.path.join(REF_ROOT, "internal", "renderers", "vanilla_2dgs_renderer.py")),
                                     reason="reference tree not present")


def _standin():
    import gspl_amd  # noqa: F401
    from gspl_amd import compat
    compat.install()
    import diff_surfel_rasterization as dsr
    if "gspl_amd" not in (dsr.__doc__ or ""):
        pytest.skip("a real diff_surfel_rasterization package is installed")
    return dsr


def test_surfel_stand_in_exposes_the_names():
    dsr = _standin()
    from gspl_amd import ops
    from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    assert GaussianRasterizer is ops.SurfelGaussianRasterizer and GaussianRasterizationSettings is ops.SurfelRasterizationSettings
    assert GaussianRasterizationSettings._fields == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier",
                                                     "viewmatrix", "projmatrix", "sh_degree", "campos", "prefiltered", "debug")
    assert dsr.GaussianRasterizer is not ops.GaussianRasterizer


def test_precomputed_transforms_are_refused():
    from gspl_amd import ops
    s = ops.SurfelRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3))
    with pytest.raises(NotImplementedError):
        ops.SurfelGaussianRasterizer(s)(torch.zeros(1, 3), torch.zeros(1, 3), torch.ones(1, 1), colors_precomp=torch.zeros(1, 3),
                                        cov3D_precomp=torch.zeros(1, 9))


def _scene(n=400, W=72, H=56, seed=3):
    means, scales, quats, opac, shs = [t.double() for t in O.synthetic_scene(n, seed=seed)]
    scales = scales * 6
    cam = O.synthetic_camera(W, H, 70.0, 68.0)
    bg = torch.tensor([0.2, 0.4, 0.1], dtype=torch.float64)
    return (means, scales, quats, opac, shs), cam, bg


def _oracle_op(calls):
    def fake(settings, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None):
        s = settings
        calls.append(dict(shs=shs is not None, colors_precomp=colors_precomp is not None, scales_shape=tuple(scales.shape)))
        r = SO.render(means3D, scales, rotations, opacities, shs, s.sh_degree, s.viewmatrix, s.projmatrix, s.campos, int(s.image_width),
                      int(s.image_height), s.bg, scale_modifier=s.scale_modifier, colors_precomp=colors_precomp)
        return r["render"], r["radii"], r["allmap"]
    return fake


class _Model:
    def __init__(self, params):
        self.get_xyz, self.get_scaling, self.get_rotation, self.get_opacity, self.get_features = params
        self.active_sh_degree = 3


@needs_reference
@pytest.mark.parametrize("form", ["shs", "colors_precomp"])
def test_reference_2dgs_renderer_runs_unedited_and_the_plugin_matches_it(monkeypatch, form):
    _standin()
    from test_package_shims import _stubs, _Cam
    _stubs()
    import gspl_amd.ops.surfel as surfel
    import internal.renderers.vanilla_2dgs_renderer as vr                       # imports from the stand-in
    import diff_surfel_rasterization as dsr
    from gspl_amd.renderers import HipVanilla2DGSRenderer
    assert vr.GaussianRasterizer is dsr.GaussianRasterizer and vr.GaussianRasterizationSettings is dsr.GaussianRasterizationSettings
    calls = []
    monkeypatch.setattr(surfel, "rasterize_surfels", _oracle_op(calls))
    # the reference's pseudo-normal helper builds its pixel grid with device='cuda'; on the CPU its device-agnostic restatement
    # (the plugin's, same arithmetic) stands in for that one static method
    monkeypatch.setattr(vr.Vanilla2DGSRenderer, "depths_to_points", staticmethod(HipVanilla2DGSRenderer.depths_to_points))
    params, cam, bg = _scene()
    kwargs = {}
    if form == "colors_precomp":
        kwargs["colors_precomp"] = torch.rand(params[0].shape[0], 3, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    model = _Model(params)
    ref_r = vr.Vanilla2DGSRenderer(depth_ratio=0.3)
    hip_r = HipVanilla2DGSRenderer(depth_ratio=0.3)
    out_ref = ref_r(_Cam(cam), model, bg, **kwargs)
    out_hip = hip_r(_Cam(cam), model, bg, **kwargs)
    assert len(calls) == 2 and calls[0] == calls[1]
    assert calls[0]["scales_shape"] == (params[0].shape[0], 2) and calls[0]["colors_precomp"] is (form == "colors_precomp")
    keys = {"render", "viewspace_points", "visibility_filter", "radii", "rend_alpha", "rend_normal", "view_normal", "rend_dist",
            "surf_depth", "surf_normal"}
    assert set(out_ref) == keys and set(out_hip) == keys
    for k in keys - {"viewspace_points"}:
        a, b = out_ref[k], out_hip[k]
        assert a.shape == b.shape, k
        if a.dtype == torch.bool or a.dtype == torch.int32:
            assert torch.equal(a, b), k
        else:
            assert float((a.double() - b.double()).abs().max()) <= 1e-9, k
    r = SO.render(*params[:4], params[4], 3, cam["world_to_camera"].double(), cam["full_projection"].double(), cam["camera_center"].double(),
                  cam["width"], cam["height"], bg, colors_precomp=kwargs.get("colors_precomp"))
    assert float((out_hip["render"] - r["render"]).abs().max()) <= 1e-12
    assert float(out_hip["rend_alpha"].max()) > 0.3 and int(out_hip["visibility_filter"].sum()) > 50
    assert {k: v.key for k, v in ref_r.get_available_outputs().items()} == {k: v.key for k, v in hip_r.get_available_outputs().items()}


def test_plugin_config_is_picklable():
    import pickle
    from gspl_amd.renderers import HipVanilla2DGSRenderer, Renderer
    r = HipVanilla2DGSRenderer(depth_ratio=1.0)
    assert isinstance(r, Renderer) and pickle.loads(pickle.dumps(r)).depth_ratio == 1.0
    assert set(r.get_available_outputs()) == {"rgb", "render_alpha", "render_normal", "view_normal", "render_dist", "surf_depth", "surf_normal"}


# ---- closed forms pinning the oracle ------------------------------------------------------------------------------------------
def _disc_scene(depths_world, quats, opac, W=33, H=33):
    cam = O.synthetic_camera(W, H, 40.0)
    n = len(depths_world)
    means = torch.tensor([[0.0, 0.0, z] for z in depths_world], dtype=torch.float64)
    scales = torch.full((n, 2), 0.3, dtype=torch.float64)
    q = torch.tensor(quats, dtype=torch.float64)
    o = torch.tensor(opac, dtype=torch.float64)[:, None]
    cp = torch.tensor([[1.0, 0.5, 0.25]] * n, dtype=torch.float64)
    bg = torch.zeros(3, dtype=torch.float64)
    r = SO.render(means, scales, q, o, None, 0, cam["world_to_camera"].double(), cam["full_projection"].double(), cam["camera_center"].double(),
                  W, H, bg, colors_precomp=cp)
    return r, cam


def test_oracle_fronto_parallel_surfel_depth_normal_distortion():
    r, cam = _disc_scene([0.0], [[1.0, 0.0, 0.0, 0.0]], [0.8])
    a = r["allmap"]
    alpha = a[1]
    hit = alpha > 1e-3
    assert int(hit.sum()) > 20
    assert float(alpha[16, 16]) == pytest.approx(0.8, abs=1e-12)        # the centre projects onto pixel (16, 16): rho = 0
    assert float((a[0][hit] / alpha[hit] - 4.0).abs().max()) < 1e-12     # depth = the plane's view depth
    assert float((a[5][hit] - 4.0).abs().max()) < 1e-12                  # median depth
    assert float((a[2:4][:, hit]).abs().max()) < 1e-12 and float((a[4][hit] / alpha[hit] + 1.0).abs().max()) < 1e-12      # -view axis
    assert float(a[6].abs().max()) < 1e-15                               # one surfel: no distortion


def test_oracle_two_surfels_distortion_closed_form():
    o1, o2 = 0.6, 0.7
    r, _ = _disc_scene([0.0, 1.0], [[1.0, 0.0, 0.0, 0.0]] * 2, [o1, o2])
    m = lambda z: SO.M_SCALE * (1 - SO.NEAR / z)
    w1, w2 = o1, o2 * (1 - o1)
    expect = w1 * w2 * (m(4.0) - m(5.0)) ** 2
    assert float(r["allmap"][6, 16, 16]) == pytest.approx(expect, rel=1e-12)
    assert float(r["allmap"][0, 16, 16]) == pytest.approx(w1 * 4.0 + w2 * 5.0, rel=1e-12)
    assert float(r["allmap"][5, 16, 16]) == pytest.approx(4.0, rel=1e-12)     # T = 0.4 after the first: the median stays there


def test_oracle_back_facing_surfel_normal_is_flipped():
    # identity rotation: world normal +z points away from the camera (which looks along +z): flipped to -z;
    # a half turn about x: world normal -z already faces the camera
    back, _ = _disc_scene([0.0], [[1.0, 0.0, 0.0, 0.0]], [0.8])
    front, _ = _disc_scene([0.0], [[0.0, 1.0, 0.0, 0.0]], [0.8])
    raw = back["pre"]["normal"]
    assert float(raw[0, 2]) == pytest.approx(-1.0) and float(front["pre"]["normal"][0, 2]) == pytest.approx(-1.0)
    assert torch.allclose(back["allmap"], front["allmap"], atol=1e-12)
    R = O.quat_to_rotmat(torch.tensor([[1.0, 0, 0, 0]], dtype=torch.float64))
    assert float(R[0, 2, 2]) == 1.0        # the unflipped view normal would have been +z

"""The PVG route, the parts that need no GPU: the declared ABI, the `nvdiffrast.torch` and `kornia.utils` stand-ins of
`gspl_amd.compat`, the refusals of the ops, the plugin's surface against the fixture tests/golden/pvg_renderer_signatures.json, and
self-checks of the fp64 oracle tests/pvg_oracle.py that tests/test_pvg_gpu.py holds the kernels to."""
import dataclasses
import inspect
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import pvg_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ROOT = os.environ.get("GSPL_REFERENCE_ROOT", "/root/reference")
needs_reference = pytest.mark.skipif(
    not os.path.exists(os.path.join(REF_ROOT, "internal", "renderers", "periodic_vibration_gaussian_renderer.py")),
    reason="reference tree not present")
NAMES = json.load(open(os.path.join(ROOT, "tests", "golden", "pvg_renderer_signatures.json")))


def test_header_declares_the_entry_points():
    from gspl_amd import _lib as L
    text = open(L.HEADER_PATH).read()
    for name in ("gspl_pvg_motion_fwd", "gspl_pvg_motion_bwd", "gspl_cubemap_fwd", "gspl_cubemap_bwd", "gspl_envlight_blend_fwd",
                 "gspl_envlight_blend_bwd"):
        assert f"int {name}(" in text and name in L.exported_symbols()
    assert L.ABI_VERSION == 39 and "17. Periodic Vibration Gaussians" in text and "PURELY\n *    ADDITIVE" in text
    assert "UNPINNED" in text[text.index("17. Periodic Vibration Gaussians"):]
    fwd, bwd = L._FUNCTIONS["gspl_pvg_motion_fwd"][2], L._FUNCTIONS["gspl_pvg_motion_bwd"][2]
    assert fwd == ("N", "means", "velocity", "t", "scale_t", "opacities", "table", "means_t", "avg_velocity", "opacity_t", "stream")
    assert bwd[-6:] == ("g_means", "g_velocity", "g_t", "g_scale_t", "g_opacities", "stream") and "means" not in bwd
    assert L._FUNCTIONS["gspl_envlight_blend_fwd"][2][-3:] == ("out", "dirs_out", "stream")
    makefile = open(os.path.join(ROOT, "gaussian-splatting-lightning_amd", "csrc", "Makefile")).read()
    assert "pvg.hip" in makefile and "envlight.hip" in makefile


def test_stand_ins_are_registered_only_for_missing_packages():
    """In a fresh interpreter: without the packages both stand-ins appear; a package that is importable is left alone."""
    code = ("import sys, types\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "real = types.ModuleType('kornia'); real.__doc__ = 'the real one'; sys.modules['kornia'] = real\n"
            "import importlib.util\n"
            "had_nvdiffrast = importlib.util.find_spec('nvdiffrast') is not None\n"
            "import gspl_amd\n"
            "from gspl_amd import compat\n"
            "installed = compat.install()\n"
            "assert sys.modules['kornia'] is real and 'kornia.utils' not in installed\n"
            "import nvdiffrast.torch as dr\n"
            "assert had_nvdiffrast or ('nvdiffrast.torch' in installed and 'gspl_amd' in dr.__doc__ and callable(dr.texture))\n"
            "assert 'nvdiffrast.torch' not in compat.install()\n"
            "del sys.modules['kornia']\n"
            "assert importlib.util.find_spec('kornia') is not None or 'kornia.utils' in compat.install()\n"
            "import kornia\n"
            "assert kornia.utils.create_meshgrid(2, 3, normalized_coordinates=False).shape == (1, 2, 3, 2)\n"
            "print('ok')\n")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stdout + res.stderr


def test_create_meshgrid_values():
    from gspl_amd import compat
    grid = compat._create_meshgrid(3, 4, normalized_coordinates=False)
    assert grid.shape == (1, 3, 4, 2) and grid.dtype == torch.float32
    assert torch.equal(grid[0, :, :, 0], torch.tensor([[0., 1., 2., 3.]] * 3)) and torch.equal(grid[0, :, :, 1], torch.tensor([[0.] * 4, [1.] * 4, [2.] * 4]))
    norm = compat._create_meshgrid(3, 5, normalized_coordinates=True, dtype=torch.float64)
    assert norm.dtype == torch.float64
    assert torch.allclose(norm[0, 0, :, 0], torch.tensor([-1., -0.5, 0., 0.5, 1.], dtype=torch.float64))
    assert torch.allclose(norm[0, :, 0, 1], torch.tensor([-1., 0., 1.], dtype=torch.float64))
    u, v = grid[0].unbind(-1)          # the reference's use: u runs along the width
    assert u.shape == (3, 4) and float(u[0, 3]) == 3 and float(v[2, 0]) == 2


def test_refusals():
    from gspl_amd import compat, ops
    base, dirs = torch.zeros(6, 4, 4, 3), torch.ones(5, 3)
    for kw in (dict(filter_mode="nearest"), dict(boundary_mode="wrap"), dict(filter_mode="linear-mipmap-linear")):
        with pytest.raises(NotImplementedError, match="linear"):
            ops.cubemap_sample(base, dirs, **kw)
    with pytest.raises(NotImplementedError, match="3 channels"):
        ops.cubemap_sample(torch.zeros(6, 4, 4, 4), dirs)
    with pytest.raises(ValueError):
        ops.cubemap_sample(torch.zeros(6, 4, 5, 3), dirs)
    with pytest.raises(ValueError):
        ops.cubemap_sample(base, torch.ones(5, 2))
    with pytest.raises(NotImplementedError, match="no gradient for the directions"):
        ops.cubemap_sample(base, dirs.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="GPU only"):          # there is no CPU fallback
        ops.cubemap_sample(base, dirs)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.envlight_blend(torch.zeros(3, 4, 5), torch.zeros(4, 5), base, torch.eye(3), 10.0, 10.0, 2.5, 2.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.pvg_motion(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 1), torch.ones(4, 1), torch.ones(4, 1), 0.5, 0.2)
    with pytest.raises(ValueError):
        ops.pvg_motion(torch.zeros(4, 2), torch.zeros(4, 3), torch.zeros(4, 1), torch.ones(4, 1), torch.ones(4, 1), 0.5, 0.2)
    # the nvdiffrast stand-in: one cube map, uv [B, H, W, 3], linear + cube, no mip-maps
    tex, uv = torch.zeros(1, 6, 4, 4, 3), torch.ones(1, 1, 5, 3)
    with pytest.raises(NotImplementedError):
        compat._texture(tex, uv)                                      # nvdiffrast's defaults: filter 'auto', boundary 'wrap'
    with pytest.raises(NotImplementedError):
        compat._texture(tex, uv, filter_mode="linear", boundary_mode="clamp")
    with pytest.raises(NotImplementedError):
        compat._texture(tex[0], uv, filter_mode="linear", boundary_mode="cube")
    with pytest.raises(NotImplementedError):
        compat._texture(tex, uv[0], filter_mode="linear", boundary_mode="cube")
    with pytest.raises(NotImplementedError):
        compat._texture(tex, uv, uv_da=torch.zeros(1), filter_mode="linear", boundary_mode="cube")
    with pytest.raises(RuntimeError, match="GPU only"):
        compat._texture(tex, uv, filter_mode="linear", boundary_mode="cube")


def test_plugin_surface_matches_the_fixture():
    from gspl_amd import renderers as R
    from gspl_amd.envlight import HipEnvLight
    config = R.HipPeriodicVibrationGaussianRenderer
    fields = dataclasses.fields(config)
    assert [f.name for f in fields] == NAMES["PeriodicVibrationGaussianRenderer"] and [f.default for f in fields] == NAMES["defaults"]
    renderer = config(env_map_res=8).instantiate()
    assert isinstance(renderer, R.HipPeriodicVibrationGaussianRendererModule) and isinstance(renderer, R.Renderer)
    renderer.setup("fit")
    assert [n for n, _ in renderer.named_buffers()] == NAMES["buffers"]
    for name in NAMES["module_methods"]:
        assert hasattr(type(renderer), name)
    assert list(inspect.signature(type(renderer).forward).parameters) == NAMES["forward_parameters"]
    assert {k: v.key for k, v in renderer.get_available_outputs().items()} == NAMES["available_outputs"]
    assert renderer.get_available_outputs()["average_velocity"].type == R.RendererOutputTypes.NORMAL_MAP
    assert renderer.get_available_outputs()["depth"].type == R.RendererOutputTypes.GRAY
    source = inspect.getsource(type(renderer).forward)
    assert all(f'"{key}"' in source for key in NAMES["output_keys"]) and str(NAMES["default_render_types"]).replace("'", '"') in source
    # the sky: the reference's parameter name, shape and initial value, so that its checkpoints load
    assert isinstance(renderer.env_map, HipEnvLight)
    state = renderer.env_map.state_dict()
    assert list(state) == NAMES["EnvLight"]["parameters"] and list(state["base"].shape) == NAMES["EnvLight"]["base_shape_for_resolution_8"]
    assert bool((state["base"] == NAMES["EnvLight"]["initial_value"]).all()) and renderer.env_map.base.requires_grad
    other = HipEnvLight(resolution=8)
    other.load_state_dict({"base": torch.rand(6, 8, 8, 3)})
    assert torch.equal(HipEnvLight.to_opengl(torch.tensor([[1., 2., 3.]])), torch.tensor([[1., 3., -2.]]))
    none = config(env_map_res=-1, lambda_self_supervision=-1).instantiate()
    none.setup("fit")
    assert none.env_map is None
    # time_interval: the reference's buffer, set by training_setup from the model's time_duration and the number of frames
    module = type("M", (), {})()
    module.gaussian_model = type("G", (), {"config": type("C", (), {"time_duration": (-0.5, 0.5)})()})()
    module.trainer = type("T", (), {"datamodule": type("D", (), {"dataparser_outputs": type("O", (), {"train_set": list(range(51))})()})()})()
    assert none.training_setup(module) == (None, None)
    assert abs(none.time_interval - 0.02) < 1e-7 and abs(float(none._time_interval) - 0.02) < 1e-7
    none._time_interval.fill_(0.5)
    assert none.time_interval == 0.5


# ---- the oracle's own checks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 4, 16])
def test_oracle_constant_texture_and_weights(R):
    dirs = PO.cubemap_directions(R).double()
    live = torch.isfinite(dirs).all(1) & ~(dirs == 0).all(1)
    texel, weight = PO.cube_taps(dirs, R)
    assert int(texel.min()) >= 0 and int(texel.max()) < 6 * R * R and bool((weight >= 0).all())
    assert float((weight.sum(1)[live] - 1).abs().max()) <= 1e-14 and not bool(weight[~live].any())
    out = PO.cubemap(torch.full((6, R, R, 3), 0.37, dtype=torch.float64), dirs)
    assert float((out[live] - 0.37).abs().max()) <= 1e-14 and not bool(out[~live].any())
    # every face is hit, and at R = 16 every kind of tap occurs: in-face, folded, dropped
    assert set(torch.unique(PO.select_face(dirs[live])[0]).tolist()) == set(range(6))
    assert int((weight[live] == 0).any(1).sum()) > 0


def test_oracle_face_table():
    """The six axes hit the centres of their faces, and (sc, tc) follow the table of the header."""
    axes = torch.tensor([[1., 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=torch.float64)
    face, sc, tc, ma = PO.select_face(axes)
    assert face.tolist() == [0, 1, 2, 3, 4, 5] and not bool(sc.any()) and not bool(tc.any()) and bool((ma == 1).all())
    p = torch.tensor([[2., 0.5, -0.25], [-2., 0.5, -0.25], [0.5, 2., -0.25], [0.5, -2., -0.25], [0.5, -0.25, 2.], [0.5, -0.25, -2.]], dtype=torch.float64)
    face, sc, tc, ma = PO.select_face(p)
    assert face.tolist() == [0, 1, 2, 3, 4, 5]
    assert sc.tolist() == [0.25, -0.25, 0.5, 0.5, 0.5, -0.5] and tc.tolist() == [-0.5, -0.5, -0.25, 0.25, 0.25, 0.25]
    # ties: |x| = |y| goes to x, |y| = |z| to y
    assert PO.select_face(torch.tensor([[1., 1., 0.5], [0.5, -1., 1.], [1., -1., -1.]], dtype=torch.float64))[0].tolist() == [0, 3, 0]
    # face_point is the inverse
    u, v = torch.tensor([0.3] * 6, dtype=torch.float64), torch.tensor([-0.7] * 6, dtype=torch.float64)
    f2, s2, t2, m2 = PO.select_face(PO.face_point(torch.arange(6), u, v, torch.ones(6, dtype=torch.float64)))
    assert f2.tolist() == list(range(6)) and torch.equal(s2, u) and torch.equal(t2, v)
    # texel (row, column) = (t, s): +x looking along -z is column 0 ... R-1
    texel, weight = PO.cube_taps(torch.tensor([[1.0, -0.75 + 1e-9, 0.75 - 1e-9]], dtype=torch.float64), 4)
    assert int(texel[0][weight[0].argmax()]) == (0 * 4 + 3) * 4 + 0          # face 0, row 3 (tc = +0.75), column 0 (sc = -0.75)


@pytest.mark.parametrize("R", [1, 2, 4, 16])
def test_oracle_is_seamless(R):
    """The value at a point exactly on an edge is the same from both faces, and at a corner from all three: approached from either
    side (the tie rule sends the point itself to one face) the sample tends to the same value."""
    g = torch.Generator().manual_seed(R)
    base = torch.rand(6, R, R, 3, generator=g, dtype=torch.float64)
    points = []
    for a in (1.0, -1.0):
        for b in (1.0, -1.0):
            for free in (-0.83, -0.31, 0.0, 0.44, 0.97, 1.0, -1.0):
                for axis in range(3):
                    p = [a, b]
                    p.insert(axis, free)
                    points.append(p)
    points = torch.tensor(points, dtype=torch.float64)
    here = PO.cubemap(base, points)
    eps = 1e-11
    for axis in range(3):          # push one coordinate out a little: the major axis changes hands
        bump = torch.zeros(3, dtype=torch.float64)
        bump[axis] = eps
        for sign in (1.0, -1.0):
            there = PO.cubemap(base, points * (1 + sign * bump))
            assert float((there - here).abs().max()) <= 1e-8 * R, (axis, sign)
    # and the faces really differ: the check above is not vacuous
    d = lambda *v: torch.tensor(v, dtype=torch.float64)
    a, b = PO.select_face(points * (1 + d(eps, 0, 0)))[0], PO.select_face(points * (1 + d(0, eps, 0)))[0]
    assert int((a != b).sum()) > 10


def test_oracle_gradient_is_the_scatter_of_the_weights():
    R = 4
    dirs = PO.cubemap_directions(R).double()
    base = torch.rand(6, R, R, 3, dtype=torch.float64, requires_grad=True)
    v = torch.randn(dirs.shape[0], 3, dtype=torch.float64)
    (grad,) = torch.autograd.grad(PO.cubemap(base, dirs), base, v)
    sums = PO.cubemap_grad_sums(R, dirs, v)
    assert bool((grad.reshape(-1, 3).abs() <= sums + 1e-12).all()) and float(sums.min()) > 0
    assert abs(float(PO.cubemap_grad_sums(R, dirs, torch.ones_like(v)).sum()) - 3 * (dirs.shape[0] - 2)) < 1e-9


def test_oracle_motion_is_the_models_getters():
    (means, velocity, t, scale_t, opac), _ = PO.motion_case(257)
    model = PO.FakePVGModel(means, torch.ones(257, 3), torch.ones(257, 4), opac, torch.zeros(257, 16, 3), velocity, t, scale_t)
    ts, shift = 0.62 - 0.5 - 0.0137, 0.0137
    want_means = model.get_mean_SHM(ts) + model.get_average_velocity() * shift
    want_opac = model.get_opacities() * model.get_marginal_t(ts)
    got = PO.motion(means, velocity, t, scale_t, opac, 0.62, -0.5, shift, 0.2, 1.0)
    assert torch.allclose(got[0], want_means, rtol=0, atol=1e-6) and torch.allclose(got[1], model.get_average_velocity(), rtol=1e-6, atol=0)
    assert torch.allclose(got[2], want_opac, rtol=1e-5, atol=0)
    dead = got[2][:, 0] == 0
    assert 0 < int(dead.sum()) < 257                       # some rows underflow, as the GPU test needs
    # the term sums bound the values
    sums, _ = PO.motion_term_sums(means, velocity, t, scale_t, opac, 0.62, -0.5, shift, 0.2, 1.0, torch.ones(257, 3), torch.ones(257, 3), torch.ones(257, 1))
    assert all(bool((g.double().abs() <= s * (1 + 1e-6) + 1e-12).all()) for g, s in zip(got, sums))          # (got is float32)
    assert PO.MARGINAL_FLOOR * PO.MIN_BOUND == 2.0 ** -126


def test_oracle_directions_and_blend():
    rot = PO.rotations()
    assert len(rot) == 6 and all(float((r @ r.T - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12 for r in rot)
    dirs = PO.pixel_directions(rot[0], 12.0, 11.5, 25.3, 18.3, 37, 50)
    assert dirs.shape == (37, 50, 3) and float((dirs.norm(dim=-1) - 1).abs().max()) < 1e-12
    # the centre pixel looks along +z of the camera, which the swap sends to +y of the map
    centre = PO.pixel_directions(rot[0], 10.0, 10.0, 0.5, 0.5, 1, 1)[0, 0]
    assert torch.allclose(centre, torch.tensor([0., 1., 0.], dtype=torch.float64))
    jitter = torch.rand(2, 37, 50, dtype=torch.float64)
    assert not torch.equal(PO.pixel_directions(rot[4], 12.0, 11.5, 25.3, 18.3, 37, 50, jitter), PO.pixel_directions(rot[4], 12.0, 11.5, 25.3, 18.3, 37, 50))
    base = torch.rand(6, 4, 4, 3, dtype=torch.float64)
    rgb, alpha = torch.rand(3, 37, 50, dtype=torch.float64), torch.rand(37, 50, dtype=torch.float64)
    alpha[3, 4] = 1.0
    out = PO.blend(rgb, alpha, base, dirs)
    assert torch.equal(out[:, 3, 4], rgb[:, 3, 4]) and float((out - rgb).min()) >= 0


@needs_reference
def test_the_references_renderer_imports_on_the_stand_ins():
    """With the stand-ins registered the reference's own PVG renderer module and its EnvLight import unedited; its
    `get_world_directions` (kornia's meshgrid) agrees with the oracle's directions before the axis swap."""
    code = ("import sys, types\n"
            f"sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
            "import torch\n"
            "import gspl_amd.renderers\n"
            "from test_package_shims import _stubs, _Cam\n"
            "_stubs()\n"
            "import importlib.util\n"
            "stand_in = 'gspl_amd' in (sys.modules.get('kornia').__doc__ or '') if 'kornia' in sys.modules else False\n"
            "from internal.renderers.periodic_vibration_gaussian_renderer import PeriodicVibrationGaussianRenderer as Ref\n"
            "import internal.model_components.envlight as envlight_module\n"
            "assert hasattr(envlight_module, 'EnvLight')\n"
            "from oracle import gsplat_oracle as O\n"
            "import pvg_oracle as PO\n"
            "cam = _Cam(O.synthetic_camera(50, 37, 12.0, 11.5))\n"
            "cam.world_to_camera = cam.world_to_camera.clone()\n"
            "cam.world_to_camera[:3, :3] = PO.rotations()[5]\n"
            "for k, v in list(vars(cam).items()):\n"
            "    if isinstance(v, torch.Tensor) and v.is_floating_point(): setattr(cam, k, v.float())          # (kornia's grid is float32)\n"
            "got = type(Ref().instantiate()).get_world_directions(cam)\n"
            "c2w = torch.linalg.inv(cam.world_to_camera.double().T)[:3, :3]\n"
            "want = PO.pixel_directions(c2w, 12.0, 11.5, 25.0, 18.5, 37, 50)\n"
            "want = torch.stack([want[..., 0], -want[..., 2], want[..., 1]], 0)\n"
            "assert got.shape == (3, 37, 50) and float((got.double() - want).abs().max()) < 1e-5, float((got.double() - want).abs().max())\n"
            "fields = [f.name for f in __import__('dataclasses').fields(Ref)]\n"
            "print('fields', fields)\n"
            "print('ok')\n")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stdout + res.stderr
    assert str(NAMES["PeriodicVibrationGaussianRenderer"]) in res.stdout

"""The SWAG route: the `tinycudann` stand-in of `gspl_amd.compat` (one class, `Encoding`, for grid encodings), the configuration
dataclasses and `HipSWAGRenderer`.  The encoding's arithmetic is held to its oracle in tests/test_hashgrid.py; here the stand-in must
be that op bit for bit, and the plugin the reference's formulation (internal/renderers/swag_renderer.py, internal/models/swag_model.py)
evaluated step by step on the same ops."""
import dataclasses
import inspect
import os
import subprocess
import sys

import pytest
import torch

from oracle import gsplat_oracle as O
from fakes import FakeCamera, FakeGaussianModel
from hip_helpers import assert_pixels_close
from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ROOT = os.environ.get("GSPL_REFERENCE_ROOT", "/root/reference")
needs_reference = pytest.mark.skipif(not os.path.exists(os.path.join(REF_ROOT, "internal", "renderers", "swag_renderer.py")),
                                     reason="reference tree not present")
DEV = "cuda:0"
SMALL = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 4, "log2_hashmap_size": 10, "base_resolution": 16, "per_level_scale": 1.5}


def _tcnn():
    from gspl_amd import compat
    compat.install()
    import tinycudann
    if "gspl_amd" not in (tinycudann.__doc__ or ""):
        pytest.skip("a real tinycudann package is installed")
    return tinycudann


# ---- no GPU ------------------------------------------------------------------------------------------------------------------------------
def test_stand_in_exposes_one_class():
    from gspl_amd import ops
    tcnn = _tcnn()
    enc = tcnn.Encoding(3, dict(SMALL, n_dims_to_encode=3))
    lv = ops.hashgrid_levels(3, 4, 4, 10, 16, 1.5)
    assert enc.n_input_dims == 3 and enc.n_output_dims == 16 == lv.n_output_dims
    assert isinstance(enc.params, torch.nn.Parameter) and enc.params.dtype == torch.float32 and enc.params.shape == (lv.n_params,)
    assert float(enc.params.detach().abs().max()) <= 1e-4 and float(enc.params.detach().abs().max()) > 5e-5
    assert [n for n, _ in enc.named_parameters()] == ["params"]
    same, other = tcnn.Encoding(3, SMALL), tcnn.Encoding(3, SMALL, seed=7)
    assert torch.equal(same.params.detach().cpu(), enc.params.detach().cpu()) and not torch.equal(other.params.detach().cpu(), enc.params.detach().cpu())
    # the alias and the dense grid; tiny-cuda-nn's documented defaults where the config is silent
    alias = tcnn.Encoding(3, {"otype": "Grid", "type": "Hash", "n_levels": 4, "n_features_per_level": 4, "log2_hashmap_size": 10, "per_level_scale": 1.5})
    assert alias.params.shape == enc.params.shape
    dense = tcnn.Encoding(2, {"otype": "DenseGrid", "n_levels": 3, "base_resolution": 4, "per_level_scale": 1.405})
    assert dense.n_output_dims == 6 and not dense.levels.hashed.any() and dense.levels.resolutions.tolist() == [4, 6, 8]
    assert tcnn.Encoding(3, {"otype": "HashGrid", "log2_hashmap_size": 8}).n_output_dims == 32
    with pytest.raises(ImportError):
        from tinycudann import Network  # noqa: F401
    assert not hasattr(tcnn, "NetworkWithInputEncoding")


def test_stand_in_refuses_what_is_not_built_by_name():
    tcnn = _tcnn()
    for config, name in (({"otype": "Frequency", "n_frequencies": 4}, "Frequency"), ({"otype": "SphericalHarmonics", "degree": 4}, "SphericalHarmonics"),
                         ({"otype": "Identity"}, "Identity"), (dict(SMALL, interpolation="Smoothstep"), "Smoothstep"),
                         ({"otype": "Grid", "type": "Tiled"}, "Tiled"), (dict(SMALL, stochastic_interpolation=True), "stochastic_interpolation"),
                         (dict(SMALL, n_dims_to_encode=2), "n_dims_to_encode")):
        with pytest.raises(NotImplementedError, match=name):
            tcnn.Encoding(3, config)
    with pytest.raises(NotImplementedError, match="float16"):
        tcnn.Encoding(3, SMALL, dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="n_input_dims"):
        tcnn.Encoding(4, SMALL)


def test_stand_in_is_registered_only_when_the_package_is_missing():
    code = ("import sys, types\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "real = types.ModuleType('tinycudann'); real.__doc__ = 'the real one'; sys.modules['tinycudann'] = real\n"
            "import importlib.util\n"
            "import gspl_amd\n"
            "from gspl_amd import compat\n"
            "installed = compat.install()\n"
            "assert sys.modules['tinycudann'] is real and 'tinycudann' not in installed\n"
            "del sys.modules['tinycudann']\n"
            "had = importlib.util.find_spec('tinycudann') is not None\n"
            "installed = compat.install()\n"
            "import tinycudann\n"
            "assert had or ('tinycudann' in installed and 'gspl_amd' in tinycudann.__doc__ and isinstance(tinycudann.Encoding, type))\n"
            "assert 'tinycudann' not in compat.install()\n"
            "print('ok')\n")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stdout + res.stderr


def test_plugin_surface():
    from gspl_amd import renderers as R, swag
    params = inspect.signature(R.HipSWAGRenderer.__init__).parameters
    assert list(params) == ["self", "network", "grid_encoding", "embedding", "optimization", "temperature", "eps"]
    assert params["temperature"].default == 0.1 and params["eps"].default == 1e-8
    assert list(inspect.signature(R.HipSWAGRenderer.forward).parameters) == ["self", "viewpoint_camera", "pc", "bg_color", "scaling_modifier", "u", "kwargs"]
    field = lambda cls: {f.name: f.default for f in dataclasses.fields(cls)}
    assert field(swag.NetworkConfig) == {"n_neurons": 64, "n_layers": 3}
    assert field(swag.EmbeddingConfig) == {"num_embeddings": 2048, "embedding_dim": 24}
    assert field(swag.GridEncodingOptimizationConfig) == {"lr": 1e-3, "max_steps": 30_000, "lr_final_factor": 0.01, "eps": 1e-15}
    assert field(swag.GridEncodingConfig) == {"type": "hashgrid", "n_frequencies": 4, "degree": 4, "n_features_per_level": 4, "log2_hashmap_size": 19,
                                              "max_resolution": 2048, "n_levels": 12, "base_resolution": 16, "per_level_scale": 1.405}
    config = swag.GridEncodingConfig().get_encoder_config(3)
    assert config["otype"] == "HashGrid" and config["n_levels"] == 12 and abs(config["per_level_scale"] - (2048 / 16) ** (1 / 11)) < 1e-12
    with pytest.raises(NotImplementedError, match="frequency"):
        swag.GridEncodingConfig(type="frequency").get_encoder_config(3)
    renderer = R.HipSWAGRenderer(grid_encoding=swag.GridEncodingConfig(n_levels=4, log2_hashmap_size=10), embedding=swag.EmbeddingConfig(num_embeddings=4))
    assert isinstance(renderer, R.Renderer)
    renderer.setup("fit", xyz=torch.tensor([[0., 1., 2.], [4., -1., 3.], [1., 0., 0.]]))
    assert renderer.bbox_min.tolist() == [0., -1., 0.] and torch.allclose(renderer.bbox_size, torch.tensor([4.4, 2.2, 3.3]))
    names = [n for n, _ in renderer.swag_model.named_parameters()]
    assert names == ["grid_encoding.params", "image_embedding.weight", "theta.0.weight", "theta.0.bias", "theta.2.weight", "theta.2.bias",
                     "theta.4.weight", "theta.4.bias"]
    assert renderer.swag_model.theta[0].in_features == 16 + 24 + 3 and renderer.swag_model.theta[4].out_features == 4
    optimizer, scheduler = renderer.training_setup(None)
    assert isinstance(optimizer, torch.optim.Adam) and len(optimizer.param_groups) == 1 and optimizer.param_groups[0]["name"] == "swag_model"
    assert optimizer.param_groups[0]["lr"] == 1e-3 and isinstance(scheduler, torch.optim.lr_scheduler.LambdaLR)
    assert abs(scheduler.lr_lambdas[0](15_000) - 0.1) < 1e-12 and scheduler.lr_lambdas[0](60_000) == 0.01
    u = renderer.uniform_sampler.sample((1,))
    assert u.shape == (1,) and 0 <= float(u) < 1


@needs_reference
def test_the_references_model_constructs_on_the_stand_in():
    """In a fresh interpreter the reference's own `SWAGModel` and `SWAGRenderer` import and construct unedited; the model's parameter
    names and shapes are `HipSWAGModel`'s, so checkpoints travel both ways."""
    code = ("import sys\n"
            f"sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
            "import torch\n"
            "import gspl_amd.renderers\n"
            "from gspl_amd import swag\n"
            "from test_package_shims import _stubs\n"
            "_stubs()\n"
            "import tinycudann\n"
            "stand_in = 'gspl_amd' in (tinycudann.__doc__ or '')\n"
            "from internal.models import swag_model as ref\n"
            "from internal.renderers.swag_renderer import SWAGRenderer\n"
            "kw = dict(n_levels=4, log2_hashmap_size=10)\n"
            "theirs = ref.SWAGModel(grid_encoding=ref.GridEncodingConfig(**kw), embedding=ref.EmbeddingConfig(num_embeddings=4))\n"
            "ours = swag.HipSWAGModel(grid_encoding=swag.GridEncodingConfig(**kw), embedding=swag.EmbeddingConfig(num_embeddings=4))\n"
            "assert not stand_in or type(theirs.grid_encoding).__module__.startswith('gspl_amd')\n"
            "a, b = theirs.state_dict(), ours.state_dict()\n"
            "assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a), (list(a), list(b))\n"
            "theirs.load_state_dict(b)\n"
            "assert SWAGRenderer().temperature == 0.1\n"
            "print('ok')\n")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stdout + res.stderr


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_stand_in_is_the_op_bit_for_bit():
    from gspl_amd import ops
    tcnn = _tcnn()
    enc = tcnn.Encoding(3, SMALL).to(DEV)
    assert enc.params.is_cuda
    x = torch.rand(1000, 3, generator=torch.Generator().manual_seed(1)).to(DEV) * 1.5 - 0.25
    with torch.no_grad():
        enc.params.mul_(1e4)
    out = enc(x)
    assert out.dtype == torch.float32 and out.shape == (1000, 16)
    assert torch.equal(out, ops.hashgrid_encode(x, enc.params.detach(), ops.hashgrid_levels(3, 4, 4, 10, 16, 1.5)))
    assert float(out.detach().abs().max()) > 0.1
    out.square().sum().backward()
    assert enc.params.grad is not None and bool(torch.isfinite(enc.params.grad).all()) and int((enc.params.grad != 0).sum()) > 1000


def _swag_scene(temperature=0.1, delta_alpha=0.75):
    from gspl_amd import renderers as R, swag
    means, scales, quats, opac, shs = O.synthetic_scene(1500, seed=5)
    cam = O.synthetic_camera(176, 128, 160.0, 158.0)
    torch.manual_seed(3)
    model = FakeGaussianModel(*[p.to(DEV) for p in (means, scales * 4, quats, opac, shs)])
    camera = FakeCamera(cam, DEV)
    camera.appearance_id = 2
    renderer = R.HipSWAGRenderer(grid_encoding=swag.GridEncodingConfig(n_levels=4, log2_hashmap_size=10), embedding=swag.EmbeddingConfig(num_embeddings=4),
                                 temperature=temperature)
    renderer.setup("fit", xyz=means)
    renderer.to(DEV)
    with torch.no_grad():          # a table that matters, and delta alpha near 0.75: a variation of ~0.05 at u = 0.5, ~0.3 at u = 0.55
        renderer.swag_model.grid_encoding.params.mul_(1e4)
        renderer.swag_model.theta[4].weight[3] *= 0.1
        renderer.swag_model.theta[4].bias[3] = delta_alpha
    return renderer, model, camera, torch.tensor([0.1, 0.3, 0.6], device=DEV)


def _step_by_step(renderer, model, camera, bg, u):
    """swag_renderer.py:41-66 and swag_model.py:98-105, one torch op per line of the reference, on the ops the plugin may use."""
    from gspl_amd import ops
    from gspl_amd.renderers.renderer import raster_settings
    m = renderer.swag_model
    xyz = model.get_xyz
    colors = torch.clamp_min(ops.spherical_harmonics(model.active_sh_degree, xyz - camera.camera_center, model.get_features) + 0.5, 0.0)
    x = (xyz.detach() - renderer.bbox_min.to(DEV)) / renderer.bbox_size.to(DEV)
    x_emb = ops.hashgrid_encode(x, m.grid_encoding.params, m.grid_encoding.levels).to(colors.dtype)
    image_emb = m.image_embedding(torch.tensor([camera.appearance_id], dtype=torch.int, device=DEV)).repeat((colors.shape[0], 1))
    output = m.theta(torch.concat([colors, x_emb, image_emb], dim=-1))
    c, delta = torch.sigmoid(output[:, :3]), output[:, -1]
    if u is None:
        u = torch.tensor(0.5, dtype=torch.float, device=DEV)
    variation = torch.sigmoid(1 / renderer.temperature * (torch.log(torch.abs(delta) + renderer.eps) + torch.log(u + renderer.eps) - torch.log(1 - u + renderer.eps)))
    final_opacity = torch.clamp_min(model.get_opacity.squeeze(-1) - variation, 0).unsqueeze(-1)
    screen = torch.zeros_like(xyz, requires_grad=True)
    image, radii = ops.GaussianRasterizer(raster_settings(camera, bg, 1.0, model.active_sh_degree))(
        means3D=xyz, means2D=screen, shs=None, colors_precomp=c, opacities=final_opacity, scales=model.get_scaling, rotations=model.get_rotation,
        cov3D_precomp=None)
    return image, radii, c, final_opacity


@pytest.mark.gpu
def test_plugin_forward_is_the_references_formulation(monkeypatch):
    from gspl_amd.renderers import hip_swag_renderer as H
    renderer, model, camera, bg = _swag_scene()
    seen = {}
    render = H.HipVanillaRenderer.render
    monkeypatch.setattr(H.HipVanillaRenderer, "render", staticmethod(lambda **kw: seen.update(kw) or render(**kw)))
    for u in (None, torch.tensor([0.55], device=DEV)):          # None: the evaluation path, u = 0.5
        with torch.no_grad():
            out = renderer(camera, model, bg, u=u)
            image, radii, colours, final_opacity = _step_by_step(renderer, model, camera, bg, u)
        assert set(out) == {"render", "depth", "viewspace_points", "visibility_filter", "radii"} and out["render"].shape == (3, 128, 176)
        assert seen["colors_precomp"].shape == (1500, 3) and seen["opacity"].shape == (1500, 1) and seen["features"] is None
        # the plugin's colours come from the fused SH launch: 1e-6 absolute on colours and opacities, then the image tolerance
        assert float((seen["colors_precomp"] - colours).abs().max()) <= 1e-6
        assert float((seen["opacity"] - final_opacity).abs().max()) <= 1e-6
        assert torch.equal(out["radii"], radii) and torch.equal(out["visibility_filter"], radii > 0)
        assert_pixels_close(out["render"].cpu().numpy(), image.cpu().numpy())
        variation = model.get_opacity.detach() - seen["opacity"]
        assert int((variation > 0.01).sum()) > 700 and int((seen["opacity"] > 0).sum()) > 300          # the variation is at work, and not everywhere fatal
    with torch.no_grad():
        assert not torch.equal(renderer(camera, model, bg)["render"], out["render"])                  # u changes the image


@pytest.mark.gpu
def test_plugin_gradients_and_two_optimizer_steps():
    # temperature 1: the variation is |delta alpha| u / (|delta alpha| u + 1 - u), which leaves splats alive for every u the step may draw
    renderer, model, camera, bg = _swag_scene(temperature=1.0, delta_alpha=0.25)
    optimizer, scheduler = renderer.training_setup(None)
    target = torch.rand(3, 128, 176, generator=torch.Generator().manual_seed(9)).to(DEV)
    out = renderer.training_forward(0, None, camera, model, bg)
    assert out["render"].shape == (3, 128, 176)
    out["viewspace_points"].retain_grad()
    (out["render"] - target).abs().mean().backward()
    m = renderer.swag_model
    named = dict(m.named_parameters(), **{f"model.{i}": p for i, p in enumerate(model.leaves())}, viewspace=out["viewspace_points"])
    for name, p in named.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), name
    rows = m.image_embedding.weight.grad.abs().sum(dim=1)
    assert float(rows[2]) > 0 and not bool(rows[[0, 1, 3]].any())          # the row of this appearance_id and no other
    # two Adam steps of the renderer's own optimizer lower a fixed photometric loss (evaluation path: u = 0.5)
    loss = lambda: (renderer(camera, model, bg)["render"] - target).abs().mean()
    with torch.no_grad():
        before = float(loss())
    for _ in range(2):
        optimizer.zero_grad(set_to_none=True)
        loss().backward()
        optimizer.step()
        scheduler.step()
    with torch.no_grad():
        after = float(loss())
    assert after < before, (before, after)


@pytest.mark.gpu
@needs_reference
def test_the_references_own_model_and_renderer_on_the_stand_in():
    """`SWAGRenderer` / `SWAGModel` are constructed unedited on the `tinycudann` stand-in (and the stand-in rasterizer); with the
    plugin's weights copied in, one forward gives the plugin's image."""
    import gspl_amd.renderers  # noqa: F401   (registers the stand-ins)
    _tcnn()
    from test_package_shims import _stubs
    _stubs()
    from internal.models import swag_model as ref_model
    from internal.renderers.swag_renderer import SWAGRenderer
    renderer, model, camera, bg = _swag_scene()
    reference = SWAGRenderer(grid_encoding=ref_model.GridEncodingConfig(n_levels=4, log2_hashmap_size=10),
                             embedding=ref_model.EmbeddingConfig(num_embeddings=4))
    reference.bbox_min, reference.bbox_size = renderer.bbox_min, renderer.bbox_size
    reference.swag_model = ref_model.SWAGModel(network=reference.network_config, grid_encoding=reference.grid_encoding_config,
                                               embedding=reference.embedding_config).to(DEV)
    assert type(reference.swag_model.grid_encoding).__module__.startswith("gspl_amd")
    reference.swag_model.load_state_dict(renderer.swag_model.state_dict())
    camera.appearance_id = 2
    with torch.no_grad():
        want = reference(camera, model, bg)
        got = renderer(camera, model, bg)
    assert_pixels_close(got["render"].cpu().numpy(), want["render"].cpu().numpy())
    assert torch.equal(got["radii"], want["radii"])

"""Renderer plugins (the drop-in boundary) on the GPU: output-dict contract of each
reference renderer they replace, parity of `render` and of the parameter gradients with the oracle,
and the consumer contract of the density controller (`viewspace_points.grad`, `.absgrad`, grad scale)."""
import numpy as np
import pytest
import torch

from oracle import gsplat_oracle as O
from fakes import FakeCamera, FakeGaussianModel
from hip_helpers import assert_close_scaled, assert_pixels_close, assert_pipeline_attributed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _scene(seed=31, n=6000, W=272, H=176):
    means, scales, quats, opac, shs = O.synthetic_scene(n, seed=seed)
    scales = scales * 4
    cam = O.synthetic_camera(W, H, 250.0, 247.0)
    g = torch.Generator().manual_seed(seed)
    wimg = torch.randn(3, H, W, generator=g)
    bg = torch.tensor([0.1, 0.3, 0.6])
    return (means, scales, quats, opac, shs), cam, wimg, bg


def _oracle_grads(api, params, cam, wimg, bg):
    W, H = cam["width"], cam["height"]
    dl = [t.double().requires_grad_(True) for t in params]
    if api == "inria":
        r = O.render_inria(*dl, 3, cam["world_to_camera"].double(), cam["full_projection"].double(), cam["camera_center"].double(),
                           cam["tanfovx"], cam["tanfovy"], W, H, bg.double())
    else:
        r = O.render_gsplat(*dl, 3, cam["world_to_camera"].double(), cam["fx"], cam["fy"], cam["cx"], cam["cy"], W, H, bg.double(),
                            cam["camera_center"].double())
    (r["render"] * wimg.double()).sum().backward()
    return r, dl


def _check(model, dl, render, r, api, cam, bg, radii=None, quats_normalised_by_renderer=False, extra=()):
    """Free-running comparison with ATTRIBUTION (hip_helpers.assert_pipeline_attributed): every pixel the oracle does
    not flag within 1e-5; every gradient element beyond 1e-4 (|ref| + rms) belongs to a splat a flagged decision reaches.
    `extra`: further (name, got, ref) per-splat gradients under the same rows (the screen-space gradient)."""
    shs_grad = torch.cat([model.shs_dc.grad, model.shs_rest.grad], dim=1)
    pairs = []
    for got, ref, name in zip([model.means.grad, model.scales_.grad, model.rotations_.grad, model.opacities_.grad, shs_grad], dl,
                              ("means", "scales", "quats", "opacities", "shs")):
        ref_g = ref.grad
        if name == "quats" and quats_normalised_by_renderer:
            # GSPlatRenderer divides the rotations by their norm (gsplat_renderer.py:68): the radial part vanishes
            q = ref.detach()
            ref_g = (ref_g - q * (q * ref_g).sum(-1, keepdim=True)) / q.norm(dim=-1, keepdim=True)
        pairs.append((name, got.cpu().numpy(), ref_g.numpy()))
    assert_pipeline_attributed(O.MODE_INRIA if api == "inria" else O.MODE_GSPLAT, r, cam["width"], cam["height"], bg.double(),
                               render.detach().cpu().numpy(), pairs + list(extra), opacities=dl[3], gpu_radii=radii)


def test_hip_vanilla_renderer_contract_and_parity():
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipVanillaRenderer
    params, cam, wimg, bg = _scene()
    model = FakeGaussianModel(*[p.to(DEV) for p in params])
    camera = FakeCamera(cam, DEV)
    renderer = HipVanillaRenderer()
    out = renderer(camera, model, bg.to(DEV))
    assert set(out) == {"render", "viewspace_points", "visibility_filter", "radii"}
    N = params[0].shape[0]
    assert out["render"].shape == (3, cam["height"], cam["width"]) and out["viewspace_points"].shape == (N, 3)
    assert out["visibility_filter"].dtype == torch.bool and out["radii"].shape == (N,)
    out["viewspace_points"].retain_grad()          # what VanillaDensityControllerImpl.before_backward does
    (out["render"] * wimg.to(DEV)).sum().backward()
    r, dl = _oracle_grads("inria", params, cam, wimg, bg)
    ref_ndc = r["xy"].grad.numpy() * np.array([0.5 * cam["width"], 0.5 * cam["height"]])
    _check(model, dl, out["render"], r, "inria", cam, bg, radii=out["radii"],
           extra=[("viewspace grad", out["viewspace_points"].grad[:, :2].cpu().numpy(), ref_ndc)])
    # depth render type (override colour path)
    d = renderer(camera, model, bg.to(DEV), render_types=["depth"])
    assert "depth" in d and d["depth"].shape == (3, cam["height"], cam["width"]) and float(d["depth"].detach().max()) > 0


def test_hip_vanilla_renderer_convert_shs_python_matches_the_default_path():
    """`convert_SHs_python=True`: the colours come from `ops.sh_view_colors(detach_means=False)` and enter the rasterizer as
    `colors_precomp`; by default the rasterizer evaluates the SH itself.  Two formulations of one function in fp32 (in the fp64
    oracle the two paths agree exactly): same image, same gradients — the means' includes the part through the view direction."""
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipVanillaRenderer
    params, cam, wimg, bg = _scene()
    camera = FakeCamera(cam, DEV)
    target = torch.rand(3, cam["height"], cam["width"], generator=torch.Generator().manual_seed(9)).to(DEV)

    def run(**kw):
        model = FakeGaussianModel(*[p.to(DEV) for p in params])
        out = HipVanillaRenderer(**kw)(camera, model, bg.to(DEV))
        (out["render"] - target).abs().mean().backward()
        return model, out

    python, out_p = run(convert_SHs_python=True)
    default, out_d = run()
    assert torch.equal(out_p["radii"], out_d["radii"])
    assert_pixels_close(out_p["render"].detach().cpu().numpy(), out_d["render"].detach().cpu().numpy(), name="convert_SHs_python render")
    for name in ("means", "shs_dc", "shs_rest"):
        assert_close_scaled(getattr(python, name).grad.cpu().numpy(), getattr(default, name).grad.cpu().numpy(), 1e-4, name)


class _RawModel(torch.nn.Module):
    """Raw parameters behind exp / normalize / sigmoid getters, as the reference's VanillaGaussianModel keeps them
    (internal/models/vanilla_gaussian.py:345-358, 421-441), declaring so (renderer.model_raw_parameters)."""
    fused_activations = {"scales": "exp", "rotations": "normalize", "opacities": "sigmoid"}

    def __init__(self, means, scales, quats, opac, shs, active_sh_degree=3, quat_norms=None):
        super().__init__()
        P = lambda t: torch.nn.Parameter(t.clone().contiguous())
        o = opac.reshape(-1, 1).clamp(1e-6, 1 - 1e-6)
        q = quats if quat_norms is None else quats * quat_norms.reshape(-1, 1)        # unnormalised, as an optimizer leaves them
        self.g = {"means": P(means), "scales": P(torch.log(scales)), "rotations": P(q), "opacities": P(torch.log(o / (1 - o))),
                  "shs_dc": P(shs[:, :1]), "shs_rest": P(shs[:, 1:])}
        self.active_sh_degree, self.max_sh_degree, self.is_pre_activated = active_sh_degree, 3, False

    def get_property(self, name): return self.g[name]
    get_xyz = property(lambda s: s.g["means"])
    get_scaling = property(lambda s: torch.exp(s.g["scales"]))
    get_rotation = property(lambda s: torch.nn.functional.normalize(s.g["rotations"]))
    get_opacity = property(lambda s: torch.sigmoid(s.g["opacities"]))
    get_features = property(lambda s: torch.cat((s.g["shs_dc"], s.g["shs_rest"]), dim=1))
    def get_shs_dc(self): return self.g["shs_dc"]
    def get_shs_rest(self): return self.g["shs_rest"]


@pytest.mark.parametrize("scaling_modifier", [1.0, 0.7])
def test_hip_vanilla_renderer_raw_parameters_activations_inside_the_kernels(scaling_modifier):
    """`fuse_activations` (GSPL_INRIA_RAW_PARAMS): the model's raw parameters go to the rasterizer, exp / normalize / sigmoid and
    their derivatives run in the preprocess kernels.  Against (1) the fp64 oracle differentiated through the same activations in
    torch fp64, (2) the same renderer with the getters left to torch."""
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipVanillaRenderer
    params, cam, wimg, bg = _scene(seed=77)
    g = torch.Generator().manual_seed(5)
    norms = 0.25 + 3.0 * torch.rand(params[0].shape[0], generator=g)
    names = ("means", "scales", "rotations", "opacities", "shs_dc", "shs_rest")
    camera = FakeCamera(cam, DEV)

    def run(fuse):
        model = _RawModel(*[p.to(DEV) for p in params], quat_norms=norms.to(DEV))
        out = HipVanillaRenderer(fuse_activations=fuse)(camera, model, bg.to(DEV), scaling_modifier=scaling_modifier)
        out["viewspace_points"].retain_grad()
        (out["render"] * wimg.to(DEV)).sum().backward()
        return model, out

    fused, out_f = run(True)
    plain, out_p = run(False)
    # (2) same kernels either way; the activations differ by at most an ulp or two (normalize: torch's reduction order)
    assert torch.equal(out_f["radii"], out_p["radii"])
    assert_pixels_close(out_f["render"].detach().cpu().numpy(), out_p["render"].detach().cpu().numpy(), tol=2e-6, name="fused vs torch activations")
    for n in names:
        assert_close_scaled(fused.g[n].grad.cpu().numpy(), plain.g[n].grad.cpu().numpy(), 1e-4, "fused vs torch: " + n, frac_ok=0.999, rel_all=0.5)
    assert_close_scaled(out_f["viewspace_points"].grad.cpu().numpy(), out_p["viewspace_points"].grad.cpu().numpy(), 1e-4, "viewspace", 0.999, rel_all=0.5)

    # (1) the oracle through torch fp64 activations
    W, H = cam["width"], cam["height"]
    raw64 = {n: fused.g[n].detach().cpu().double().requires_grad_(True) for n in names}
    r = O.render_inria(raw64["means"], torch.exp(raw64["scales"]), torch.nn.functional.normalize(raw64["rotations"]),
                       torch.sigmoid(raw64["opacities"]).reshape(-1), torch.cat((raw64["shs_dc"], raw64["shs_rest"]), dim=1), 3,
                       cam["world_to_camera"].double(), cam["full_projection"].double(), cam["camera_center"].double(),
                       cam["tanfovx"], cam["tanfovy"], W, H, bg.double(), scale_modifier=scaling_modifier)
    (r["render"] * wimg.double()).sum().backward()
    # (a radius is a ceil of an fp32 expression of fp32 exp(raw): one in a few thousand may sit on an integer within an ulp)
    assert float((out_f["radii"].cpu() == torch.as_tensor(r["radii"]).to(torch.int32)).float().mean()) >= 0.999
    assert_pipeline_attributed(O.MODE_INRIA, r, W, H, bg.double(), out_f["render"].detach().cpu().numpy(),
                               [("vs oracle: " + n, fused.g[n].grad.cpu().numpy(), raw64[n].grad.numpy()) for n in names],
                               opacities=torch.sigmoid(raw64["opacities"]).reshape(-1), gpu_radii=out_f["radii"])


def test_raw_parameters_need_a_zeroed_state_and_the_scale_rotation_pair(monkeypatch):
    import ctypes
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib as L, ops
    from gspl_amd.ops import _frame
    params, cam, wimg, bg = _scene(n=500)
    m, s, q, o, sh = [p.to(DEV) for p in params]
    settings = ops.GaussianRasterizationSettings(cam["height"], cam["width"], cam["tanfovx"], cam["tanfovy"], bg.to(DEV), 1.0,
                                                 cam["world_to_camera"].to(DEV), cam["full_projection"].to(DEV), 3, cam["camera_center"].to(DEV))
    cov = torch.zeros(500, 6, device=DEV)
    with pytest.raises(Exception, match="scale/rotation"):
        ops.GaussianRasterizer(settings)(m, torch.zeros_like(m), o, shs=sh, cov3D_precomp=cov, raw_parameters=True)
    # the C boundary itself: unknown flag bits are refused before anything is launched
    state = L.InriaState()
    state.flags = 64
    out, radii = torch.empty(3, cam["height"], cam["width"], device=DEV), torch.empty(500, dtype=torch.int32, device=DEV)

    def refuse(nbytes, device, tag):      # (a block asked for before the refusal would end the call with this error instead)
        raise MemoryError("no block")

    monkeypatch.setattr(_frame, "allocate", refuse)
    with pytest.raises(Exception, match="flags"), _frame.FrameBlocks(DEV) as frame:
        L.call("gspl_rasterize_inria_fwd", 500, 3, 16, L.ptr(m), L.ptr(s), L.ptr(q), None, L.ptr(sh), None, None, L.ptr(o),
               L.ptr(settings.viewmatrix), L.ptr(settings.projmatrix), L.ptr(settings.campos), L.ptr(settings.bg), cam["width"], cam["height"],
               float(cam["tanfovx"]), float(cam["tanfovy"]), 1.0, frame.callback, None, 0, L.ptr(out), L.ptr(radii), ctypes.byref(state), L.stream(), None)


def test_config1_lego_proxy_800x800_100k_vanilla_renderer_vs_oracle():
    """BASELINE.json configs[0]/[1] proxy (S-800-100k: 100 000 Gaussians of the Blender init box at 800x800, SH degree 3,
    vanilla renderer) end to end against the fp64 oracle: render within 1e-5, every parameter gradient within 1e-4."""
    import gspl_amd  # noqa: F401
    from gspl_amd import synthetic
    from gspl_amd.renderers import HipVanillaRenderer
    wl = synthetic.WORKLOADS["S-800-100k"]
    params = O.synthetic_scene(wl["n"], seed=42)
    cam = O.synthetic_camera(wl["width"], wl["height"], wl["fx"])
    g = torch.Generator().manual_seed(1)
    wimg = torch.randn(3, wl["height"], wl["width"], generator=g)
    bg = torch.zeros(3)
    model = FakeGaussianModel(*[p.to(DEV) for p in params])
    out = HipVanillaRenderer()(FakeCamera(cam, DEV), model, bg.to(DEV))
    out["viewspace_points"].retain_grad()
    (out["render"] * wimg.to(DEV)).sum().backward()
    r, dl = _oracle_grads("inria", params, cam, wimg, bg)
    _check(model, dl, out["render"], r, "inria", cam, bg, radii=out["radii"])
    assert int(out["visibility_filter"].sum()) > 90_000          # the survey measured V = 94 935 with the reference's projection


@pytest.mark.parametrize("which", ["v0", "v1", "v1-tile-culling"])
def test_hip_gsplat_renderers_contract_and_parity(which):
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipGSplatRenderer, HipGSplatV1Renderer
    params, cam, wimg, bg = _scene(seed=32)
    model = FakeGaussianModel(*[p.to(DEV) for p in params])
    camera = FakeCamera(cam, DEV)
    renderer = HipGSplatRenderer(absgrad=True) if which == "v0" else \
        HipGSplatV1Renderer(tile_based_culling=(which == "v1-tile-culling")).instantiate()
    out = renderer(camera, model, bg.to(DEV))
    for k in ("render", "viewspace_points", "viewspace_points_grad_scale", "visibility_filter", "radii"):
        assert k in out
    N, W, H = params[0].shape[0], cam["width"], cam["height"]
    assert out["viewspace_points"].shape == (N, 2)
    assert torch.allclose(out["viewspace_points_grad_scale"].cpu(), 0.5 * torch.tensor([[W, H]], dtype=torch.float32))
    out["viewspace_points"].retain_grad()
    (out["render"] * wimg.to(DEV)).sum().backward()
    r, dl = _oracle_grads("gsplat", params, cam, wimg, bg)
    vp = out["viewspace_points"]
    _check(model, dl, out["render"], r, "gsplat", cam, bg, radii=out["radii"], quats_normalised_by_renderer=(which == "v0"),
           extra=[("xys.grad", vp.grad.cpu().numpy(), r["xys"].grad.numpy())])
    assert hasattr(vp, "absgrad") and torch.all(vp.absgrad >= vp.grad.abs() - 1e-6)
    if which != "v0":
        # `acc_vis` (the fork's has_hit_any_pixels, set by the rasterizer FORWARD: gsplat_v1_renderer.py:287): present before any
        # backward, and exactly the splats some pixel composites — checked against the per-splat hit-pixel counts of the same
        # lists (gspl_composite_scores, itself checked against the oracle in tests/test_scores.py)
        from gspl_amd import ops
        acc = out["acc_vis"]
        assert acc is not None and acc.dtype == torch.bool and acc.shape == (N,)
        _, _, flat, offs = out["isects"]
        _, m2, _, conics, _ = out["projections"]
        count = ops.composite_scores(m2.reshape(N, 2), conics.reshape(N, 3), out["opacities"].reshape(N), W, H, 16, offs, flat)[0]
        assert torch.equal(acc, count > 0)
        assert not bool((acc & ~out["visibility_filter"]).any()) and 0 < int(acc.sum()) < int(out["visibility_filter"].sum())


def test_hip_pypreprocess_renderer_contract_and_parity():
    """Stand-in for `PythonPreprocessGSplatRenderer` (BASELINE.json configs[0], pypreprocess_gsplat_renderer.py:8-66): its output
    dictionary (scalar grad scale, projection mask) and parity of render + gradients with the oracle's gsplat pipeline."""
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipPythonPreprocessGSplatRenderer
    params, cam, wimg, bg = _scene(seed=34)
    model = FakeGaussianModel(*[p.to(DEV) for p in params])
    renderer = HipPythonPreprocessGSplatRenderer()
    assert renderer.block_size == 16 and renderer.anti_aliased is True
    out = renderer(FakeCamera(cam, DEV), model, bg.to(DEV))
    assert set(out) == {"render", "viewspace_points", "viewspace_points_grad_scale", "visibility_filter", "radii"}
    W, H = cam["width"], cam["height"]
    assert out["viewspace_points_grad_scale"] == 0.5 * max(H, W) and out["render"].shape == (3, H, W)
    out["viewspace_points"].retain_grad()
    (out["render"] * wimg.to(DEV)).sum().backward()
    r, dl = _oracle_grads("gsplat", params, cam, wimg, bg)
    assert torch.equal(out["visibility_filter"].cpu(), r["mask"])
    _check(model, dl, out["render"], r, "gsplat", cam, bg, radii=out["radii"],
           extra=[("xys.grad", out["viewspace_points"].grad.cpu().numpy(), r["xys"].grad.numpy())])


@pytest.mark.parametrize("model_name", ["fisheye", "ortho"])
def test_v1_renderer_runtime_camera_model(model_name):
    """The viewer's camera-model dropdown (gsplat_v1_renderer.py:653-661) sets `runtime_options.camera_model`; the projection
    then runs the fisheye / ortho model.  Render and every parameter gradient against the oracle pipeline with the same model."""
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipGSplatV1Renderer
    W, H = 272, 176
    means, scales, quats, opac, shs = O.synthetic_scene(6000, seed=33)
    if model_name == "fisheye":
        scales = scales * 4
        cam = O.synthetic_camera(W, H, 110.0, 108.0, distance=2.5)        # ~100 degrees across the image
    else:
        scales = scales * 4
        cam = O.synthetic_camera(W, H, 70.0, 69.0, distance=4.0)          # 70 pixels per world unit
    params = (means, scales, quats, opac, shs)
    g = torch.Generator().manual_seed(3)
    wimg = torch.randn(3, H, W, generator=g)
    bg = torch.tensor([0.2, 0.1, 0.4])
    model = FakeGaussianModel(*[p.to(DEV) for p in params])
    renderer = HipGSplatV1Renderer().instantiate()
    renderer.runtime_options.camera_model = model_name
    out = renderer(FakeCamera(cam, DEV), model, bg.to(DEV))
    assert int(out["visibility_filter"].sum()) > 3000
    (out["render"] * wimg.to(DEV)).sum().backward()
    dl = [t.double().requires_grad_(True) for t in params]
    r = O.render_gsplat(*dl, 3, cam["world_to_camera"].double(), cam["fx"], cam["fy"], cam["cx"], cam["cy"], W, H, bg.double(),
                        cam["camera_center"].double(), camera_model=model_name)
    (r["render"] * wimg.double()).sum().backward()
    _check(model, dl, out["render"], r, "gsplat", cam, bg, radii=out["radii"])
    # and it is not the pinhole image
    pin = HipGSplatV1Renderer().instantiate()(FakeCamera(cam, DEV), FakeGaussianModel(*[p.to(DEV) for p in params]), bg.to(DEV))
    assert float((pin["render"] - out["render"]).abs().max()) > 0.05


def test_hip_gsplat_renderer_depth_types():
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipGSplatRenderer, HipGSplatV1Renderer
    params, cam, wimg, bg = _scene(seed=33, n=3000)
    model = FakeGaussianModel(*[p.to(DEV) for p in params])
    camera = FakeCamera(cam, DEV)
    H, W = cam["height"], cam["width"]
    types = ["rgb", "alpha", "acc_depth", "acc_depth_inverted", "exp_depth", "exp_depth_inverted", "inverse_depth", "hard_depth",
             "hard_inverse_depth"]
    for renderer in (HipGSplatRenderer(), HipGSplatV1Renderer().instantiate()):
        with torch.no_grad():
            out = renderer(camera, model, bg.to(DEV), render_types=types)
        assert out["render"].shape == (3, H, W)
        for k in ("alpha", "acc_depth", "acc_depth_inverted", "exp_depth", "exp_depth_inverted", "inverse_depth", "hard_depth",
                  "hard_inverse_depth"):
            assert out[k].shape == (1, H, W), k
            assert torch.isfinite(out[k]).all(), k
        a = out["alpha"]
        assert float(a.min()) >= 0 and float(a.max()) <= 1
        covered = a[0] > 0.5
        # expected depth = acc_depth / alpha lies inside the scene's depth range where coverage is high
        ed = out["exp_depth"][0][covered]
        assert float(ed.min()) > 2.0 and float(ed.max()) < 6.0
    v1 = HipGSplatV1Renderer().instantiate()
    with torch.no_grad():
        o = v1(camera, model, bg.to(DEV), render_types=["rgb", "normal", "acc_depth"])       # 7 feature channels in one pass
    assert o["normal"].shape == (3, H, W) and o["acc_depth"].shape == (1, H, W)


def test_distributed_renderer_world1_matches_v1():
    """World size 1: the Gaussian-sharded renderer (batched projection -> packed records -> composite) must
    reproduce the staged v1 renderer; per-camera xys receive the gradient the density controller reads."""
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipGSplatDistributedRenderer, HipGSplatV1Renderer
    params, cam, wimg, bg = _scene(seed=34, n=5000)
    camera = FakeCamera(cam, DEV)
    m1 = FakeGaussianModel(*[p.to(DEV) for p in params])
    m2 = FakeGaussianModel(*[p.to(DEV) for p in params])
    ref = HipGSplatV1Renderer().instantiate()(camera, m1, bg.to(DEV))
    out = HipGSplatDistributedRenderer().instantiate()(camera, m2, bg.to(DEV))
    assert set(out) == {"render", "hard_inverse_depth", "cameras", "projection_results_list", "visible_mask_list", "xys_grad_scale_required"}
    assert torch.allclose(out["render"], ref["render"], atol=2e-6)
    (out["render"] * wimg.to(DEV)).sum().backward()
    (ref["render"] * wimg.to(DEV)).sum().backward()
    for a, b in zip(m2.leaves(), m1.leaves()):
        assert_close_scaled(a.grad.cpu().numpy(), b.grad.cpu().numpy(), 2e-5, "grad", frac_ok=0.999, rel_all=1e-3)
    xys = out["projection_results_list"][0][1]
    assert xys.grad is not None and xys.grad.shape == (params[0].shape[0], 2)


@pytest.mark.parametrize("culling,exchange", [(False, "counted"), (True, "counted"), (True, "padded")])
def test_distributed_renderer_three_node_step_equals_the_staged_one(culling, exchange):
    """`fused_step` (ops.sharded_front / sharded_exchange / sharded_back: three autograd nodes) launches the same kernels on the same
    buffers as the stage-by-stage formulation: the image and every forward output are bit-identical, the gradients differ by the
    run-to-run spread of the compositing backward's atomics only, and the per-camera xys gradient (what the distributed density
    controller reads) arrives through the exchange node's tap.  Two frames: the second one runs on a speculative list length."""
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipGSplatDistributedRenderer
    params, cam, wimg, bg = _scene(seed=36, n=5000)
    camera = FakeCamera(cam, DEV)
    models = [FakeGaussianModel(*[p.to(DEV) for p in params]) for _ in range(2)]
    renderers = [HipGSplatDistributedRenderer(tile_based_culling=culling, fused_step=f, exchange=exchange).instantiate() for f in (True, False)]
    for frame in range(2):
        outs = []
        for model, renderer in zip(models, renderers):
            for t in model.leaves():
                t.grad = None
            out = renderer(camera, model, bg.to(DEV))
            out["projection_results_list"][0][1].retain_grad()
            (out["render"] * wimg.to(DEV)).sum().backward()
            outs.append(out)
        fused, staged = outs
        assert renderers[0].last_exchange == renderers[1].last_exchange == exchange
        assert torch.equal(fused["render"], staged["render"])
        for a, b in zip(fused["projection_results_list"][0], staged["projection_results_list"][0]):
            assert torch.equal(a.detach(), b.detach())
        ga, gb = fused["projection_results_list"][0][1].grad, staged["projection_results_list"][0][1].grad
        assert ga is not None and float((ga - gb).abs().max()) <= 1e-5 * float(gb.abs().max()) + 1e-12
        for k, (a, b) in enumerate(zip(models[0].leaves(), models[1].leaves())):
            tol = 1e-4 if k < 3 else 1e-5           # means, scales, rotations sit behind the conic -> covariance chain (test_rccl_single_rank)
            assert a.grad is not None and float((a.grad - b.grad).abs().max()) <= tol * float(b.grad.abs().max()) + 1e-12, (frame, k)


def test_distributed_renderer_subclass_colours_are_used():
    """A subclass that overrides `get_rgbs(pc, camera, projection_results)` — the reference's appearance-embedding variant does
    (gsplat_distributed_appearance_embedding_renderer.py:67-84) — supplies the colours in batched mode too, and its colours take
    part in autograd."""
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipGSplatDistributedRenderer, HipGSplatDistributedRendererImpl
    params, cam, wimg, bg = _scene(seed=35, n=3000)
    model = FakeGaussianModel(*[p.to(DEV) for p in params])
    tint = torch.tensor([0.9, 0.2, 0.1], device=DEV, requires_grad=True)
    calls = []

    class Tinted(HipGSplatDistributedRendererImpl):
        def get_rgbs(self, pc, camera, projection_results):
            calls.append(projection_results[-1].shape)
            base = HipGSplatDistributedRendererImpl.get_rgbs(self, pc, camera, projection_results)
            return base * tint

    plain = HipGSplatDistributedRenderer().instantiate()(FakeCamera(cam, DEV), model, bg.to(DEV))["render"].detach()
    out = Tinted(HipGSplatDistributedRenderer())(FakeCamera(cam, DEV), model, bg.to(DEV))["render"]
    assert calls == [(3000,)] and float((out[1] - plain[1]).abs().max()) > 0.05      # green channel scaled by 0.2
    out.sum().backward()
    assert tint.grad is not None and float(tint.grad.abs().sum()) > 0


def test_concurrent_streams_are_reentrant():
    """The viewer situation (SURVEY §8b threads/streams): several host threads, each on its own stream, render concurrently
    under no_grad.  Every frame must equal the single-thread frame bit for bit (scratch is per call; the sort and scan kernels of
    concurrent frames share the device and never wait for one another)."""
    import threading
    import gspl_amd  # noqa: F401
    from gspl_amd import ops, synthetic
    wl = synthetic.WORKLOADS["S-800-100k"]
    cam = synthetic.camera(wl["width"], wl["height"], wl["fx"], distance=4.0)
    m, s_, q, o, c = [t.to(DEV) for t in synthetic.scene(wl["n"], seed=42)]
    settings = ops.GaussianRasterizationSettings(
        image_height=wl["height"], image_width=wl["width"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=torch.zeros(3, device=DEV),
        scale_modifier=1.0, viewmatrix=cam["world_to_camera"].to(DEV), projmatrix=cam["full_projection"].to(DEV), sh_degree=3,
        campos=cam["camera_center"].to(DEV))
    rast = ops.GaussianRasterizer(settings)

    def frame():
        with torch.no_grad():
            return rast(means3D=m, means2D=torch.empty_like(m), opacities=o, shs=c, scales=s_, rotations=q)[0]

    ref = frame().clone()
    torch.cuda.synchronize()
    bad = []

    def worker():
        st = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(st):
            for _ in range(12):
                if not torch.equal(frame(), ref):
                    bad.append(1)
            st.synchronize()

    threads = [threading.Thread(target=worker) for _ in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not bad


def test_gsplat_renderer_sees_pose_updates_and_other_devices_current():
    """The per-camera view-matrix cache is keyed on the pose tensor's identity and version: an in-place pose update (pose
    refinement, viewer edits) changes the render.  And a render with tensors on cuda:0 is unaffected by what the caller's
    current device is (checked with the guard's bookkeeping: one device on the test boxes)."""
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib as L
    from gspl_amd.renderers import HipGSplatRenderer
    params, cam, wimg, bg = _scene(seed=35, n=2000)
    model = FakeGaussianModel(*[p.to(DEV) for p in params])
    camera = FakeCamera(cam, DEV)
    r = HipGSplatRenderer()
    with torch.no_grad():
        a = r(camera, model, bg.to(DEV))["render"].clone()
        b = r(camera, model, bg.to(DEV))["render"]
        assert torch.equal(a, b)
        camera.world_to_camera[3, 0] += 0.25                       # in place: same tensor object, new version
        c = r(camera, model, bg.to(DEV))["render"]
        assert float((a - c).abs().max()) > 1e-3
        camera.world_to_camera = camera.world_to_camera.clone()    # replaced: same values
        d = r(camera, model, bg.to(DEV))["render"]
        assert torch.equal(c, d)
    # the same for the v1 renderer's per-camera (view matrix, K) cache and for the cached image size / field of view
    from gspl_amd.renderers import HipGSplatV1Renderer, HipVanillaRenderer
    for make in (lambda: HipGSplatV1Renderer().instantiate(), lambda: HipVanillaRenderer()):
        camera = FakeCamera(cam, DEV)
        r = make()
        with torch.no_grad():
            a = r(camera, model, bg.to(DEV))["render"].clone()
            assert torch.equal(a, r(camera, model, bg.to(DEV))["render"])
            camera.world_to_camera[3, 0] += 0.25
            if hasattr(camera, "full_projection"):
                camera.full_projection = camera.world_to_camera @ (torch.linalg.inv(FakeCamera(cam, DEV).world_to_camera) @ FakeCamera(cam, DEV).full_projection)
            c = r(camera, model, bg.to(DEV))["render"].clone()
            assert float((a - c).abs().max()) > 1e-3
            camera.fx.mul_(1.1), camera.fy.mul_(1.1)                   # intrinsics in place (the vanilla path reads the fov instead)
            camera.fov_x.mul_(0.9), camera.fov_y.mul_(0.9)
            e = r(camera, model, bg.to(DEV))["render"]
            assert float((c - e).abs().max()) > 1e-3
            H0 = int(camera.height)
            camera.height = torch.tensor(H0 - 16, dtype=camera.height.dtype, device=DEV)      # replaced size field
            assert r(camera, model, bg.to(DEV))["render"].shape[1] == H0 - 16
    g = L.device_guard(params[0].to(DEV))
    with g:
        assert g.prev == -1 and torch.cuda.current_device() == 0      # already current: nothing switched, nothing to restore


@pytest.mark.parametrize("block_size", [8, 32])
def test_renderers_accept_the_reference_block_size_field(block_size):
    """`block_size` is a configuration field of the reference's gsplat renderers (gsplat_renderer.py:6,34-43,
    gsplat_v1_renderer.py:23-41) that selects the tile side of ITS rasterizer; the image and the gradients do not depend on it.
    The renderers here keep the field (checkpoint hparams) and render on 16 x 16 tiles: the same bits as block_size = 16, forward
    and backward, for the v0 and the v1 plugin."""
    import warnings
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipGSplatRenderer, HipGSplatV1Renderer
    params, cam, wimg, bg = _scene(n=3000)
    camera = FakeCamera(cam, DEV)

    def run(make):
        model = FakeGaussianModel(*[p.to(DEV) for p in params])
        out = make()(camera, model, bg.to(DEV))
        (out["render"] * wimg.to(DEV)).sum().backward()
        return out["render"].detach(), model.means.grad.clone(), model.opacities_.grad.clone()

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for make16, makeB in ((lambda: HipGSplatV1Renderer(block_size=16).instantiate(), lambda: HipGSplatV1Renderer(block_size=block_size).instantiate()),
                              (lambda: HipGSplatRenderer(block_size=16), lambda: HipGSplatRenderer(block_size=block_size))):
            a, b = run(make16), run(makeB)
            assert torch.equal(a[0], b[0])                                   # the image: bit-identical
            for x, y in zip(a[1:], b[1:]):                                   # gradients: the same kernels on the same lists (fp32 atomics order only)
                assert_close_scaled(y.cpu().numpy(), x.cpu().numpy(), 1e-4, "gradient", frac_ok=1.0)
    assert HipGSplatV1Renderer(block_size=block_size).block_size == block_size      # the field itself is kept
    assert any("16 x 16" in str(w.message) for w in caught) or block_size == 16


@pytest.mark.parametrize("which", ["gsplat_v0", "vanilla"])
def test_more_list_entries_than_the_library_holds_is_a_python_exception_naming_the_limit(which):
    """VERDICT r3 / BASELINE configs[4] scale: every list path of the library indexes its per-tile lists with 32-bit positions and
    sorts at most 2^30-1 records.  A frame beyond that (here 140 000 screen-filling splats x 8160 tiles = 1.14e9 intersections —
    only the COUNT half of the binning runs, nothing of that size is allocated) must surface from the renderer's forward as an
    exception that names the limit, on both plugin families."""
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipGSplatRenderer, HipVanillaRenderer
    from gspl_amd import synthetic
    n, W, H = 140_000, 1920, 1080
    g = torch.Generator().manual_seed(0)
    means = (torch.rand(n, 3, generator=g) - 0.5) * 0.02                      # all in front of the camera, near the axis
    scales = torch.full((n, 3), 8.0)                                          # projected radius far beyond the image
    quats = torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(n, 1)
    opac = torch.full((n, 1), 0.5)
    shs = torch.zeros(n, 16, 3)
    model = FakeGaussianModel(*[t.to(DEV) for t in (means, scales, quats, opac, shs)])
    camera = FakeCamera(synthetic.camera(W, H, 1600.0), DEV)
    renderer = HipGSplatRenderer() if which == "gsplat_v0" else HipVanillaRenderer()
    with pytest.raises(RuntimeError, match=r"2\^30-1"):
        with torch.no_grad():
            renderer(camera, model, torch.zeros(3, device=DEV))
    # and the next, ordinary frame is unaffected
    small = FakeGaussianModel(*[t[:2000].to(DEV) for t in (means, scales * 0.001, quats, opac, shs)])
    with torch.no_grad():
        out = renderer(camera, small, torch.zeros(3, device=DEV))
    assert torch.isfinite(out["render"]).all()

"""`gspl_amd.renderers.HipGSplatMipSplattingRendererV2` and `HipGSplatAppearanceEmbeddingMipRenderer` on a small fake of the reference's
`MipSplattingModel` (defined here: raw scales and opacities, a `filter_3d` property, the reference's getters): the plugin's whole forward
and backward against `HipGSplatV1Renderer` fed the reference's expression for the filtered scales and opacities in float32 torch ops,
the appearance-Mip hooks against the same expression, forty Adam steps with a filter recomputation in the middle, and a render type
without RGB.

Tolerances are those of the assembled-pipeline tests (tests/test_glossy_renderer_gpu.py): `assert_pixels_close` (at least 99.9 % of the
pixels within 1e-5, all within 4e-3: one flipped 1/255 decision, the two sides' opacities differ by float32 rounding); gradients at
least 99.5 % of the elements within 1e-4 (|ref| + rms), none beyond 0.05 but a counted handful (8), none beyond 0.5."""
import types

import pytest
import torch

from fakes import FakeCamera
from hip_helpers import assert_close_scaled, assert_pixels_close
from oracle import gsplat_oracle as O
from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H, N = 64, 48, 3000
TAIL, OUTLIERS = 0.05, 8


class FakeMipModel(torch.nn.Module):
    """The surface of internal/models/mip_splatting.py + vanilla_gaussian.py the renderers touch: RAW `scales` (log) and `opacities`
    (logit) with the vanilla activations, `filter_3d` [N, 1] without a gradient, `config.opacity_compensation`.  In `ReferenceNamedMipModel` the
    activation methods and getters carry the module and qualified names of the reference's classes, which is what the plugin looks
    at before it hands the kernel the raw parameters; this class itself goes through the getters."""

    def __init__(self, means, scales, quats, opac, shs, filter_3d, opacity_compensation=True, active_sh_degree=3, n_feature_dims=0):
        super().__init__()
        P = torch.nn.Parameter
        self.gaussians = {"means": P(means), "shs_dc": P(shs[:, :1].contiguous()), "shs_rest": P(shs[:, 1:].contiguous()),
                          "opacities": P(torch.logit(opac.reshape(-1, 1).clamp(1e-4, 1 - 1e-4))), "scales": P(torch.log(scales)), "rotations": P(quats),
                          "filter_3d": P(filter_3d.reshape(-1, 1), requires_grad=False)}
        if n_feature_dims:
            g = torch.Generator().manual_seed(21)
            self.gaussians["appearance_features"] = P((torch.randn(means.shape[0], n_feature_dims, generator=g) * 0.5).to(means.device))
        self.config = types.SimpleNamespace(opacity_compensation=opacity_compensation)
        self.active_sh_degree = active_sh_degree
        self.is_pre_activated = False

    properties = property(lambda s: s.gaussians)
    get_xyz = property(lambda s: s.gaussians["means"])
    n_gaussians = property(lambda s: s.gaussians["means"].shape[0])

    def get_property(self, name): return self.gaussians[name]
    def get_means(self): return self.gaussians["means"]
    def get_rotations(self): return torch.nn.functional.normalize(self.gaussians["rotations"])
    def get_shs_dc(self): return self.gaussians["shs_dc"]
    def get_shs_rest(self): return self.gaussians["shs_rest"]
    def get_appearance_features(self): return self.gaussians["appearance_features"]
    def get_3d_filter(self): return self.gaussians["filter_3d"].detach()
    def scale_activation(self, scales): return torch.exp(scales)
    def opacity_activation(self, opacities): return torch.sigmoid(opacities)
    def get_scales(self): return self.scale_activation(self.gaussians["scales"])
    def get_opacities(self): return self.opacity_activation(self.gaussians["opacities"])

    def leaves(self):
        return {k: v for k, v in self.gaussians.items() if v.requires_grad}


class ReferenceNamedMipModel(FakeMipModel):
    """the same arithmetic under the reference's names (see FakeMipModel)"""


for _name, _module, _owner in (("scale_activation", "internal.models.vanilla_gaussian", "VanillaGaussianModel"),
                               ("opacity_activation", "internal.models.vanilla_gaussian", "VanillaGaussianModel"),
                               ("get_scales", "internal.models.gaussian", "GaussianModel"), ("get_opacities", "internal.models.gaussian", "GaussianModel")):
    _fn = types.FunctionType(getattr(FakeMipModel, _name).__code__, globals(), _name)
    _fn.__module__, _fn.__qualname__ = _module, f"{_owner}.{_name}"
    setattr(ReferenceNamedMipModel, _name, _fn)


def torch_filtered(model):
    """`MipSplattingUtils.apply_3d_filter` restated in float32 torch ops on the getters -> (opacities [N, 1] or the coefficient-free
    ones, scales, coef)"""
    scales, filter_3d = model.get_scales(), model.get_3d_filter()
    scales_square = torch.square(scales)
    scales_after_square = scales_square + torch.square(filter_3d)
    coef = torch.sqrt(scales_square.prod(dim=1) / scales_after_square.prod(dim=1))
    opacities = model.get_opacities()
    if model.config.opacity_compensation:
        opacities = opacities * coef[..., None]
    return opacities, torch.sqrt(scales_after_square), coef


def _torch_module(**config):
    from gspl_amd.renderers import HipGSplatV1Renderer, HipGSplatV1RendererModule

    class TorchMipModule(HipGSplatV1RendererModule):
        def get_scales(self, camera, gaussian_model, **kwargs):
            opacities, scales, _ = torch_filtered(gaussian_model)
            return scales, opacities.squeeze(-1)

        def get_opacities(self, camera, gaussian_model, projections, visibility_filter, status, **kwargs):
            return status, None

    return TorchMipModule(HipGSplatV1Renderer(filter_2d_kernel_size=0.1, **config))


def _scene(seed=43, filter_scale=1.0):
    means, scales, quats, opac, shs = O.synthetic_scene(N, seed=seed)
    g = torch.Generator().manual_seed(seed)
    filter_3d = filter_scale * (0.002 + 0.03 * torch.rand(N, generator=g))      # of the size of the scales: the filter matters
    cam = O.synthetic_camera(W, H, 60.0, 59.0)
    wimg = torch.randn(3, H, W, generator=g)
    return (means, scales * 4, quats, opac, shs, filter_3d), cam, wimg, torch.tensor([0.1, 0.3, 0.6])


def _model(params, cls=FakeMipModel, **kw):
    return cls(*[p.to(DEV) for p in params], **kw)


@pytest.mark.parametrize("cls", [FakeMipModel, ReferenceNamedMipModel], ids=["getters", "raw"])
@pytest.mark.parametrize("compensation,anti_aliased", [(True, True), (False, True), (True, False)])
def test_forward_and_backward_against_the_torch_expression(monkeypatch, cls, compensation, anti_aliased):
    from gspl_amd import ops
    from gspl_amd.renderers import HipGSplatMipSplattingRendererV2
    params, cam, wimg, bg = _scene()
    camera = FakeCamera(cam, DEV)
    seen, real = [], ops.mip_apply_3d_filter
    monkeypatch.setattr(ops, "mip_apply_3d_filter", lambda *a, **k: seen.append(k) or real(*a, **k))
    runs = {}
    for name, module in (("hip", HipGSplatMipSplattingRendererV2(anti_aliased=anti_aliased).instantiate()), ("torch", _torch_module(anti_aliased=anti_aliased))):
        model = _model(params, cls, opacity_compensation=compensation)
        out = module(camera, model, bg.to(DEV))
        (out["render"] * wimg.to(DEV)).sum().backward()
        runs[name] = (out, model)
    raw = cls is ReferenceNamedMipModel
    assert len(seen) == 1 and seen[0]["raw_scales"] is raw and seen[0]["raw_opacities"] is raw and seen[0]["opacity_compensation"] is compensation
    (out, model), (ref_out, ref_model) = runs["hip"], runs["torch"]
    assert tuple(out["render"].shape) == (3, H, W) and int(out["visibility_filter"].sum()) > N // 2
    assert_pixels_close(out["render"].detach().cpu().numpy(), ref_out["render"].detach().cpu().numpy())
    assert float((out["scales"] - ref_out["scales"]).detach().abs().max()) <= 1e-6 * float(ref_out["scales"].detach().max())
    for name, leaf in model.leaves().items():
        ref = ref_model.leaves()[name].grad
        assert leaf.grad is not None and ref is not None and tuple(leaf.grad.shape) == tuple(leaf.shape), name
        assert_close_scaled(leaf.grad.cpu().numpy(), ref.cpu().numpy(), 1e-4, name, frac_ok=0.995, rel_all=TAIL, outliers=OUTLIERS)
        assert bool(ref.any()), name
    assert model.gaussians["filter_3d"].grad is None
    # the filter is felt: without it the image differs
    plain = _model(params[:5] + (torch.zeros(N),), cls)
    with torch.no_grad():
        other = HipGSplatMipSplattingRendererV2(anti_aliased=anti_aliased).instantiate()(camera, plain, bg.to(DEV))["render"]
    assert float((other - out["render"]).abs().max()) > 1e-2


@pytest.mark.parametrize("cls", [FakeMipModel, ReferenceNamedMipModel], ids=["getters", "raw"])
@pytest.mark.parametrize("compensation", [True, False])
def test_appearance_mip_hooks_against_the_torch_expression(cls, compensation):
    """`get_scales` -> (filtered scales, coef); `get_opacities` multiplies the appearance renderer's opacities by it when the model's
    config says so (during the warm-up those are the model's own), values and gradients."""
    from gspl_amd import appearance as A, renderers as R
    params, cam, _, bg = _scene()
    camera = FakeCamera(cam, DEV)
    camera.appearance_id = torch.tensor(1, dtype=torch.int, device=DEV)
    torch.manual_seed(3)
    module = R.HipGSplatAppearanceEmbeddingMipRenderer(model=A.ModelConfig(n_appearances=3), optimization=A.OptimizationConfig(warm_up=10)).instantiate()
    module._setup_model(device=DEV)
    assert module.config.filter_2d_kernel_size == 0.1
    g = torch.Generator().manual_seed(8)
    vs, vo = torch.randn(N, 3, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)
    visible = torch.ones(N, dtype=torch.bool, device=DEV)
    grads = {}
    for side in ("hip", "torch"):
        model = _model(params, cls, opacity_compensation=compensation, n_feature_dims=64)
        if side == "hip":
            scales, status = module.get_scales(camera, model)
            assert (status is None) == (not compensation)
            opacities, rgbs = module.get_opacities(camera, model, None, visible, status, warm_up=True)
            assert tuple(rgbs.shape) == (N, 3)
        else:
            filtered, scales, coef = torch_filtered(model)
            opacities = filtered.squeeze(-1)
        ((scales * vs).sum() + (opacities * vo).sum()).backward()
        grads[side] = (scales.detach(), opacities.detach(), model.gaussians["scales"].grad, model.gaussians["opacities"].grad)
    for name, got, want in zip(("scales", "opacities", "v_scales", "v_opacities"), grads["hip"], grads["torch"]):
        assert got.shape == want.shape, name
        assert_close_scaled(got.cpu().numpy(), want.cpu().numpy(), 1e-4, name)          # (no discrete decision here: every element)
    # ... and the whole plugin renders after the warm-up, the coefficient in its opacities
    model = _model(params, cls, opacity_compensation=compensation, n_feature_dims=64)
    out = module.training_forward(100, None, camera, model, bg.to(DEV))
    want = torch_filtered(model)[0].squeeze(-1)
    assert tuple(out["render"].shape) == (3, H, W) and bool(torch.isfinite(out["render"]).all())
    compensations = out["projections"][4][0]          # (anti_aliased: the projection's 2D compensation is on top)
    assert float((out["opacities"] - want * compensations).abs().max()) <= 1e-5


def test_forty_steps_of_adam_with_a_filter_recomputation():
    """The training loop's shape: the model's own optimiser on scales and opacities, `compute_3d_filter` at step 20 only.  The loss
    falls, and the filter changes at that step and at no other."""
    from gspl_amd import mip, ops
    from gspl_amd.renderers import HipGSplatMipSplattingRendererV2
    params, cam, _, bg = _scene()
    camera, module = FakeCamera(cam, DEV), HipGSplatMipSplattingRendererV2().instantiate()
    table = ops.mip_camera_table([camera], DEV)
    assert tuple(table.shape) == (1, 16)
    target_model = _model(params)
    target_model.gaussians["filter_3d"] = mip.compute_3d_filter([camera], target_model)
    with torch.no_grad():
        target = module(camera, target_model, bg.to(DEV))["render"].clone()
    model = _model(params[:1] + (params[1] * 0.6, params[2], params[3] * 0.5) + params[4:])
    model.gaussians["filter_3d"] = mip.compute_3d_filter(None, model, camera_table=table)
    assert torch.equal(model.get_3d_filter(), target_model.get_3d_filter())          # the same means, the same camera
    opt = torch.optim.Adam([{"name": k, "params": [model.gaussians[k]], "lr": lr} for k, lr in (("scales", 0.02), ("opacities", 0.02), ("means", 0.002))])
    losses, changed = [], []
    for step in range(40):
        before = model.get_3d_filter().clone()
        if step == 20:
            model.gaussians["filter_3d"] = mip.compute_3d_filter(None, model, camera_table=table)
        out = module(camera, model, bg.to(DEV))
        loss = (out["render"] - target).abs().mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
        changed.append(not torch.equal(before, model.get_3d_filter()))
    losses = torch.stack(losses).cpu()
    print(f"loss {float(losses[0]):.5f} -> {float(losses[-1]):.5f}; filter changed at steps {[i for i, c in enumerate(changed) if c]}")
    assert bool(torch.isfinite(losses).all()) and all(bool(torch.isfinite(p).all()) for p in model.gaussians.values())
    assert float(losses[-1]) < float(losses[0]) and changed == [step == 20 for step in range(40)]


def test_render_types_without_rgb_take_the_filtered_opacities(monkeypatch):
    from gspl_amd import ops
    from gspl_amd.renderers import HipGSplatMipSplattingRendererV2
    params, cam, _, bg = _scene()
    camera, model = FakeCamera(cam, DEV), _model(params)
    calls, real = [], ops.mip_apply_3d_filter
    monkeypatch.setattr(ops, "mip_apply_3d_filter", lambda *a, **k: calls.append(1) or real(*a, **k))
    with torch.no_grad():
        out = HipGSplatMipSplattingRendererV2().instantiate()(camera, model, bg.to(DEV), render_types=["acc_depth"])
        ref = _torch_module()(camera, model, bg.to(DEV), render_types=["acc_depth"])
        plain = _torch_module()(camera, _model(params[:5] + (torch.zeros(N),)), bg.to(DEV), render_types=["acc_depth"])
    assert calls == [1] and out["render"] is None and tuple(out["acc_depth"].shape) == (1, H, W)
    scale = float(ref["acc_depth"].max())
    assert scale > 1.0
    assert_pixels_close((out["acc_depth"] / scale).cpu().numpy(), (ref["acc_depth"] / scale).cpu().numpy(), name="acc_depth")
    assert float((plain["acc_depth"] - ref["acc_depth"]).abs().max()) / scale > 1e-3          # (the filtered opacities are felt here too)

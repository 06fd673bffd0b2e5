"""HipGSplatAppearanceEmbeddingRenderer on the GPU: the warm-up is the staged gsplat-v1 plugin bit for bit; after it the fused MLP
(`fused_mlp=True`) and the torch path (`fused_mlp=False`) of the same parameters give the same image (1e-5) and the same gradients
(every element within 1e-4 (|ref| + rms(ref)) of its tensor, the torch path being `ref`); the embedding gradient touches the camera's
row only; a Gaussian behind the camera gets no colour and no feature gradient; the step adds no host synchronisation to the v1
plugin's; and forty steps on two differently tinted targets lower the loss and separate the two embedding rows."""
import warnings

import pytest
import torch

from oracle import gsplat_oracle as O
from fakes import FakeCamera, FakeGaussianModel
from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, W, H, IDS = 300, 64, 48, 3
BEHIND = 17          # this Gaussian sits behind the camera


class AppearanceGaussianModel(FakeGaussianModel):
    def __init__(self, *args, n_feature_dims=64, **kw):
        super().__init__(*args, **kw)
        g = torch.Generator().manual_seed(21)
        self.appearance_features = torch.nn.Parameter((torch.randn(self.means.shape[0], n_feature_dims, generator=g) * 0.5).to(self.means.device))

    n_gaussians = property(lambda s: s.means.shape[0])

    def get_appearance_features(self): return self.appearance_features
    def leaves(self): return super().leaves() + [self.appearance_features]


def _scene(appearance_id=1, **model_options):
    from gspl_amd import appearance as A, renderers as R
    means, scales, quats, opac, shs = O.synthetic_scene(N, seed=5)
    means[BEHIND] = torch.tensor([0.1, 0.1, -6.0])
    model = AppearanceGaussianModel(*[p.to(DEV) for p in (means, scales * 8, quats, opac * 0.8, shs)])
    camera = FakeCamera(O.synthetic_camera(W, H, 60.0, 59.0), DEV)
    camera.appearance_id = torch.tensor(appearance_id, dtype=torch.int, device=DEV)
    renderers = []
    for fused in (True, False):
        torch.manual_seed(3)
        module = R.HipGSplatAppearanceEmbeddingRenderer(model=A.ModelConfig(n_appearances=IDS, **model_options), fused_mlp=fused,
                                                        optimization=A.OptimizationConfig(warm_up=10)).instantiate()
        module._setup_model(device=DEV)
        module.train()
        renderers.append(module)
    renderers[1].load_state_dict(renderers[0].state_dict())
    return model, camera, renderers, torch.tensor([0.1, 0.3, 0.6], device=DEV)


def _weights():
    return torch.rand(3, H, W, generator=torch.Generator().manual_seed(9)).to(DEV)


def _step(renderer, model, camera, bg, step=100):
    """One training forward and backward of a fixed linear loss -> (image, {name: gradient})."""
    for p in list(model.parameters()) + list(renderer.parameters()):
        p.grad = None
    out = renderer.training_forward(step, None, camera, model, bg)
    (out["render"] * _weights()).sum().backward()
    grads = {name: p.grad.clone() for name, p in model.named_parameters() if p.grad is not None}
    grads.update({"renderer." + name: p.grad.clone() for name, p in renderer.named_parameters() if p.grad is not None})
    return out, grads


def test_warm_up_is_the_v1_plugin_bit_for_bit():
    """Two runs are compared bit for bit, so the compositing backward adds its rows in list order (`ops.set_deterministic`), not by
    atomics in dispatch order."""
    from gspl_amd import ops, renderers as R
    model, camera, (fused, _), bg = _scene()
    plain = R.HipGSplatV1Renderer().instantiate()
    before = ops.set_deterministic(True)
    try:
        got, got_grads = _step(fused, model, camera, bg, step=9)
        want, want_grads = _step(plain, model, camera, bg, step=9)
        after, _ = _step(fused, model, camera, bg, step=10)
    finally:
        ops.set_deterministic(before)
    assert torch.equal(got["render"], want["render"]) and torch.equal(got["radii"], want["radii"])
    names = [n for n in want_grads]
    assert names and set(names) == {n for n in got_grads if not n.startswith("renderer.")} and "appearance_features" not in got_grads
    assert [n for n in names if not torch.equal(got_grads[n], want_grads[n])] == []
    assert not any(n.startswith("renderer.") for n in got_grads)          # the network takes no part before the warm-up ends
    assert not torch.equal(after["render"], want["render"])


@pytest.mark.parametrize("options", [dict(), dict(is_view_dependent=True), dict(normalize=True), dict(with_opacity=True)],
                         ids=["view_independent", "view_dependent", "normalize", "with_opacity"])
def test_fused_against_the_torch_path(options):
    model, camera, (fused, torch_path), bg = _scene(**options)
    assert fused.model.uses_fused(model.appearance_features) and not torch_path.model.uses_fused(model.appearance_features)
    got, got_grads = _step(fused, model, camera, bg)
    want, want_grads = _step(torch_path, model, camera, bg)
    assert torch.equal(got["radii"], want["radii"]) and int(want["visibility_filter"].sum()) > N // 2
    image_error = float((got["render"].detach() - want["render"].detach()).abs().max())
    print(f"image max |fused - torch| = {image_error:.3e}")
    assert image_error <= 1e-5
    expected = {"means", "opacities_", "shs_dc", "shs_rest", "appearance_features", "renderer.model.embedding.weight"} | \
        {f"renderer.model.network.output_layers.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")}
    assert expected <= set(want_grads) and set(got_grads) == set(want_grads)
    for name in sorted(want_grads):
        ref = want_grads[name].double()
        bound = 1e-4 * (ref.abs() + ref.pow(2).mean().sqrt())
        worst = float(((got_grads[name].double() - ref).abs() / bound.clamp_min(1e-300)).max())
        print(f"{name}: max error / bound = {worst:.3e}")
        assert worst <= 1.0, name
        assert bool(ref.any()), name
    rows = got_grads["renderer.model.embedding.weight"].abs().sum(dim=1)
    assert float(rows[1]) > 0 and not bool(rows[[0, 2]].any())          # the row of the camera's id and no other
    if options.get("with_opacity"):
        assert fused.opacity_offsets.shape == (N,) and int(fused.opacity_offsets_count) == int(want["visibility_filter"].sum())
        assert not bool(fused.opacity_offsets[~want["visibility_filter"]].any())
        host = type("Host", (), {"device": DEV, "batch_size": 1, "log": lambda self, *a, **kw: None})()
        reg = fused.opacity_offset_reg(None, None, model, 100, host)
        mean = fused.opacity_offsets[want["visibility_filter"]].mean() * 0.05
        assert abs(float(reg) - float(mean)) <= 1e-6


def test_a_gaussian_behind_the_camera_gets_no_colour_and_no_gradient():
    model, camera, (fused, _), bg = _scene(with_opacity=True)
    out, grads = _step(fused, model, camera, bg)
    visible = out["visibility_filter"]
    assert not bool(visible[BEHIND]) and int(out["radii"][BEHIND]) == 0
    assert not bool(grads["appearance_features"][BEHIND].any()) and bool(grads["appearance_features"][visible].any())
    with torch.no_grad():
        rgbs, opacities, offsets = fused._get_rgbs_and_opacities(camera, model, out["projections"], visible, None)
    assert not bool(rgbs[BEHIND].any()) and float(offsets[BEHIND]) == 0 and float(opacities[BEHIND]) == float(model.get_opacities()[BEHIND, 0])
    assert not bool(rgbs[~visible].any()) and bool(rgbs[visible].any()) and float(rgbs.min()) >= 0 and float(rgbs.max()) <= 1


def _sync_warnings(renderer, model, camera, bg):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            _step(renderer, model, camera, bg)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    return len([w for w in caught if "synchroniz" in str(w.message).lower()])


def test_no_host_synchronisation_is_added():
    """The appearance stage itself (SH, MLP, offsets, clamp; forward and backward) runs under torch's sync debug mode "error"; the
    whole step warns no more often than the v1 plugin's (whose forward copies one host scalar to the device)."""
    from gspl_amd import renderers as R
    model, camera, (fused, _), bg = _scene(is_view_dependent=True, with_opacity=True)
    plain = R.HipGSplatV1Renderer().instantiate()
    out, _ = _step(fused, model, camera, bg)          # (loads the kernels)
    _step(plain, model, camera, bg)
    visible, projections = out["visibility_filter"], out["projections"]
    colour_weights, opacity_weights = torch.rand(N, 3, device=DEV), torch.rand(N, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rgbs, opacities, offsets = fused._get_rgbs_and_opacities(camera, model, projections, visible, None)
        ((rgbs * colour_weights).sum() + (opacities * opacity_weights).sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert bool(model.appearance_features.grad.any())
    assert _sync_warnings(fused, model, camera, bg) <= _sync_warnings(plain, model, camera, bg)


def test_forty_steps_on_two_tinted_targets():
    model, camera, (fused, _), bg = _scene()
    fused.config.optimization.warm_up = 0
    with torch.no_grad():
        base = _plain_image(model, camera, bg)
        fused.model.embedding.weight[1] = fused.model.embedding.weight[0]          # the two rows start equal
        initial = fused.model.embedding.weight.clone()
    targets = {0: (base * torch.tensor([1.0, 0.7, 0.7], device=DEV).view(3, 1, 1)).clamp(0, 1),
               1: (base * torch.tensor([0.7, 0.7, 1.0], device=DEV).view(3, 1, 1)).clamp(0, 1)}
    optimizers, schedulers = fused.training_setup(type("Host", (), {"extra_train_metrics": []})())
    optimizers.append(torch.optim.Adam([model.appearance_features], lr=5e-3))
    ids = {i: torch.tensor(i, dtype=torch.int, device=DEV) for i in targets}
    losses = []
    for step in range(40):
        camera.appearance_id = ids[step % 2]
        for optimizer in optimizers:
            optimizer.zero_grad(set_to_none=True)
        loss = (fused.training_forward(step, None, camera, model, bg)["render"] - targets[step % 2]).abs().mean()
        loss.backward()
        for optimizer in optimizers:
            optimizer.step()
        for scheduler in schedulers:
            scheduler.step()
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu()
    assert bool(torch.isfinite(losses).all())
    assert float(losses[-4:].mean()) < float(losses[:4].mean()), losses.tolist()
    rows = fused.model.embedding.weight.detach()
    assert float((rows[0] - rows[1]).abs().max()) > 1e-3 and torch.equal(rows[2], initial[2])


def _plain_image(model, camera, bg):
    from gspl_amd import renderers as R
    return R.HipGSplatV1Renderer().instantiate()(camera, model, bg)["render"]

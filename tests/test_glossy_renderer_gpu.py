"""`gspl_amd.renderers.HipGlossyRenderer` on a small fake of the reference's `GlossyGaussianModel` (defined here): the plugin's whole
forward and backward against the same plugin with the reference's expression for the opacities in float32 torch ops, and a short
optimisation of `opacity_rest`.

Tolerances are those of the assembled-pipeline tests (tests/test_metric_point_parity.py): at least 99.9 % of the pixels within 1e-5 and
all within 4e-3 (one flipped 1/255 decision: the two sides' opacities differ by float32 rounding); gradients at least 99.5 % of the
elements within 1e-4 (|ref| + rms), none beyond 0.05 but a counted handful (8), none beyond 0.5."""
import numpy as np
import pytest
import torch

import glossy_oracle as GO
from fakes import FakeCamera
from hip_helpers import assert_close_scaled, assert_pixels_close
from oracle import gsplat_oracle as O
from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H, N = 64, 48, 3000
TAIL, OUTLIERS = 0.05, 8


class FakeGlossyModel(torch.nn.Module):
    """The surface of internal/models/glossy_gaussian.py the renderer and the density controller touch: `properties` (raw opacity
    coefficients `opacities` [N, 1, 1] and `opacity_rest` [N, Kr, 1]), the v1 getters, `get_opacities` (the degree-0 activation) and
    `update_opacity_max` as the reference writes it.  Scales and rotations are stored activated."""

    def __init__(self, means, scales, quats, opac, shs, opacity_rest, active_sh_degree=3):
        super().__init__()
        P = torch.nn.Parameter
        self.gaussians = {"means": P(means), "shs_dc": P(shs[:, :1].contiguous()), "shs_rest": P(shs[:, 1:].contiguous()),
                          "opacities": P(((opac.reshape(-1, 1, 1) - 0.5) / GO.C0).contiguous()), "opacity_rest": P(opacity_rest.contiguous()),
                          "scales": P(scales), "rotations": P(quats),
                          "opacity_max": torch.zeros(means.shape[0], device=means.device)}
        self.active_sh_degree = active_sh_degree
        self.is_pre_activated = False

    properties = property(lambda s: s.gaussians)
    get_xyz = property(lambda s: s.gaussians["means"])

    def get_means(self): return self.gaussians["means"]
    def get_scales(self): return self.gaussians["scales"]
    def get_rotations(self): return self.gaussians["rotations"]
    def get_shs_dc(self): return self.gaussians["shs_dc"]
    def get_shs_rest(self): return self.gaussians["shs_rest"]
    def get_opacities(self): return GO.C0 * self.gaussians["opacities"][..., 0, :] + 0.5
    def get_opacity_max(self): return self.gaussians["opacity_max"]

    def update_opacity_max(self, new_opacities):
        with torch.no_grad():
            self.gaussians["opacity_max"] = torch.maximum(self.get_opacities().squeeze(-1), new_opacities)

    def leaves(self):
        return {k: v for k, v in self.gaussians.items() if isinstance(v, torch.nn.Parameter)}


def torch_view_opacities(degree, means, camera_center, dc, rest):
    """`GlossyRendererModule.get_opacities` restated: F.normalize -> `eval_sh_decomposed` (degrees 0 .. 3, its forms) + 0.5 -> clamp."""
    d = torch.nn.functional.normalize(means.detach() - camera_center, dim=-1)
    result = GO.C0 * dc[..., 0, :]
    if degree > 0:
        x, y, z = d[..., 0:1], d[..., 1:2], d[..., 2:3]
        result = result - GO.C1 * y * rest[..., 0, :] + GO.C1 * z * rest[..., 1, :] - GO.C1 * x * rest[..., 2, :]
    if degree > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        result = (result + GO.C2[0] * xy * rest[..., 3, :] + GO.C2[1] * yz * rest[..., 4, :] + GO.C2[2] * (2.0 * zz - xx - yy) * rest[..., 5, :]
                  + GO.C2[3] * xz * rest[..., 6, :] + GO.C2[4] * (xx - yy) * rest[..., 7, :])
    if degree > 2:
        result = (result + GO.C3[0] * y * (3 * xx - yy) * rest[..., 8, :] + GO.C3[1] * xy * z * rest[..., 9, :]
                  + GO.C3[2] * y * (4 * zz - xx - yy) * rest[..., 10, :] + GO.C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * rest[..., 11, :]
                  + GO.C3[4] * x * (4 * zz - xx - yy) * rest[..., 12, :] + GO.C3[5] * z * (xx - yy) * rest[..., 13, :]
                  + GO.C3[6] * x * (xx - 3 * yy) * rest[..., 14, :])
    assert degree <= 3
    return torch.clamp((result + 0.5).squeeze(-1), min=0., max=1.)


def _torch_module(**config):
    from gspl_amd.renderers import HipGSplatV1Renderer, HipGSplatV1RendererModule

    class TorchGlossyModule(HipGSplatV1RendererModule):
        def get_opacities(self, camera, gaussian_model, projections, visibility_filter, status, **kwargs):
            p = gaussian_model.properties
            return torch_view_opacities(gaussian_model.active_sh_degree, gaussian_model.get_xyz, camera.camera_center, p["opacities"],
                                        p["opacity_rest"]), status

    return TorchGlossyModule(HipGSplatV1Renderer(**config))


def _scene(seed=41, rest_scale=0.3):
    means, scales, quats, opac, shs = O.synthetic_scene(N, seed=seed)
    g = torch.Generator().manual_seed(seed)
    rest = rest_scale * torch.randn(N, 15, 1, generator=g)
    cam = O.synthetic_camera(W, H, 60.0, 59.0)
    wimg = torch.randn(3, H, W, generator=g)
    return (means, scales * 4, quats, opac, shs, rest), cam, wimg, torch.tensor([0.1, 0.3, 0.6])


def _model(params):
    return FakeGlossyModel(*[p.to(DEV) for p in params])


def test_the_torch_restatement_is_the_oracle():
    """(so that the comparisons below are against the pinned arithmetic)"""
    params, cam, _, _ = _scene()
    model = _model(params)
    center = cam["camera_center"].to(DEV)
    got = torch_view_opacities(3, model.get_xyz.double(), center.double(), model.properties["opacities"].double(), model.properties["opacity_rest"].double())
    o = GO.opacity(3, params[0].numpy(), cam["camera_center"].numpy(), model.properties["opacities"].detach().cpu().numpy().reshape(-1),
                   params[5].numpy()[..., 0])
    assert np.abs(got.detach().cpu().numpy() - o["value"]).max() <= 1e-12


@pytest.mark.parametrize("anti_aliased,tile_based_culling", [(True, False), (False, False), (True, True)])
def test_forward_and_backward_against_the_torch_expression(anti_aliased, tile_based_culling):
    """Anti-aliasing compensation on and off, and configs/glossy.yaml's own setting (tile-based culling, which reads the opacities)."""
    from gspl_amd.renderers import HipGlossyRenderer
    params, cam, wimg, bg = _scene()
    camera = FakeCamera(cam, DEV)
    runs, config = {}, dict(anti_aliased=anti_aliased, tile_based_culling=tile_based_culling)
    for name, module in (("hip", HipGlossyRenderer(**config).instantiate()), ("torch", _torch_module(**config))):
        model = _model(params)
        out = module(camera, model, bg.to(DEV))
        (out["render"] * wimg.to(DEV)).sum().backward()
        runs[name] = (out, model)
    (out, model), (ref_out, ref_model) = runs["hip"], runs["torch"]
    assert tuple(out["render"].shape) == (3, H, W)
    assert_pixels_close(out["render"].detach().cpu().numpy(), ref_out["render"].detach().cpu().numpy())
    for name, leaf in model.leaves().items():
        ref = ref_model.leaves()[name].grad
        assert leaf.grad is not None and ref is not None and tuple(leaf.grad.shape) == tuple(leaf.shape), name
        assert_close_scaled(leaf.grad.cpu().numpy(), ref.cpu().numpy(), 1e-4, name, frac_ok=0.995, rel_all=TAIL, outliers=OUTLIERS)
        assert bool(ref.any()), name
    # every row is evaluated: the density controller's running maximum reads the invisible ones too
    visible, opacities = out["visibility_filter"], out["opacities"]
    assert tuple(opacities.shape) == (N,) and 0 < int(visible.sum()) < N
    if not anti_aliased:                       # (with the compensation on, invisible rows are multiplied by a compensation of 0)
        want = torch_view_opacities(3, model.get_xyz, camera.camera_center, model.properties["opacities"], model.properties["opacity_rest"])
        assert float((opacities - want).detach().abs().max()) <= 1e-5 and bool((opacities[~visible] > 0).any())
        model.update_opacity_max(opacities)
        assert tuple(model.get_opacity_max().shape) == (N,) and bool((model.get_opacity_max() >= opacities.detach()).all())


def test_render_types_without_rgb_take_the_hip_opacities(monkeypatch):
    from gspl_amd import ops
    from gspl_amd.renderers import HipGlossyRenderer
    params, cam, _, bg = _scene()
    camera, model = FakeCamera(cam, DEV), _model(params)
    calls, real = [], ops.sh_view_opacities
    monkeypatch.setattr(ops, "sh_view_opacities", lambda *a, **k: calls.append(1) or real(*a, **k))
    with torch.no_grad():
        out = HipGlossyRenderer().instantiate()(camera, model, bg.to(DEV), render_types=["acc_depth"])
        ref = _torch_module()(camera, model, bg.to(DEV), render_types=["acc_depth"])
    assert calls == [1] and out["render"] is None and tuple(out["acc_depth"].shape) == (1, H, W)
    scale = float(ref["acc_depth"].max())
    assert scale > 1.0
    assert_pixels_close((out["acc_depth"] / scale).cpu().numpy(), (ref["acc_depth"] / scale).cpu().numpy(), name="acc_depth")


def test_forty_steps_of_adam_on_opacity_rest():
    """The reference's extra optimiser: torch.optim.Adam on `opacity_rest` alone.  The target is a frame of the same scene with non-zero
    view dependence; the trained model starts without any."""
    from gspl_amd.renderers import HipGlossyRenderer
    params, cam, _, bg = _scene(rest_scale=0.8)
    camera, module = FakeCamera(cam, DEV), HipGlossyRenderer().instantiate()
    with torch.no_grad():
        target = module(camera, _model(params), bg.to(DEV))["render"].clone()
    model = _model(params[:5] + (torch.zeros_like(params[5]),))
    rest = model.properties["opacity_rest"]
    opt = torch.optim.Adam([{"name": "opacity_rest", "params": [rest]}], lr=0.02)
    losses = []
    for _ in range(40):
        out = module(camera, model, bg.to(DEV))
        loss = (out["render"] - target).abs().mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        model.update_opacity_max(out["opacities"])
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu()
    print(f"loss {float(losses[0]):.5f} -> {float(losses[-1]):.5f}; |opacity_rest| max {float(rest.detach().abs().max()):.3f}")
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(rest).all()) and bool(torch.isfinite(model.get_opacity_max()).all())
    assert float(losses[-1]) < float(losses[0]) and float(rest.detach().abs().max()) > 0

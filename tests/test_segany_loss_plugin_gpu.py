"""`gspl_amd.segany.use_hip_loss` on the GPU: one training step of a module with the attributes of `SegAnySplatting` through
`HipGSplatContrastiveFeatureRenderer` and `use_hip_smoothing`, against the fp64 oracle tests/segany_loss_oracle.py fed with the step's
recorded draws (the locked-selection rule and the counted bounds of tests/test_segany_loss.py).

The oracle starts at the rendered map.  The gradient it gives for that map is compared texel by texel; the gradient of
`gaussian_semantic_features` is compared with the oracle's map gradient pulled back through the same renderer and smoothing, within
the project's gradient tolerance (1e-4 of |ref| + rms, as tests/test_smooth_features.py has it); the gate's Linear by the chain rule in
float64."""
import types

import numpy as np
import pytest
import torch

import segany_loss_oracle as SG
from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)
from test_segany_loss import EPS, _within

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_POINTS, W, H, C = 3000, 97, 65, 32
MASK_HW = (40, 60)


def _module(scale_aware_dim, mask_scales):
    from fakes import FakePropertyModel
    from gspl_amd.renderers import HipGSplatContrastiveFeatureRenderer
    from gspl_amd.segany import use_hip_loss, use_hip_smoothing
    from oracle import gsplat_oracle as O
    means, scales, quats, opac, shs = O.synthetic_scene(N_POINTS, seed=11)
    model = FakePropertyModel(*[t.to(DEV) for t in (means, scales * 3, quats, opac, shs)])
    for p in model.properties.values():
        p.requires_grad_(False)

    class Module(torch.nn.Module):                    # the attributes of SegAnySplatting that the step reads
        def __init__(self):
            super().__init__()
            self.gaussian_semantic_features = torch.nn.Parameter(torch.randn(N_POINTS, C, generator=torch.Generator().manual_seed(3)).to(DEV))
            self.scale_gate = torch.nn.Sequential(torch.nn.Linear(1, C, bias=True), torch.nn.Sigmoid()).to(DEV)
            self.bg_color = torch.zeros(C, device=DEV)
            self.models = types.SimpleNamespace(gaussian=model)
            self.smooth_K, self.smooth_dropout = 16, 0.5
            self.renderer = HipGSplatContrastiveFeatureRenderer()
            self.scale_aware_dim, self.ray_sample_rate, self.num_sampled_rays, self.rfn = scale_aware_dim, 0, 160, 1.0
            self.upper_bound_scale = float(mask_scales.max())
            self.q_trans = lambda s: (s / (1 + s)).reshape(-1, 1)
            if 0 < scale_aware_dim < 32:              # the reference's table: row i has 32 - scale_aware_dim + i ones in front
                self.fixed_scale_gate = (torch.arange(32)[None, :] < (32 - scale_aware_dim + torch.arange(scale_aware_dim + 1))[:, None]).long().to(DEV)

        def forward(self, camera):
            out = self.renderer(camera, self.models.gaussian, self.bg_color, semantic_features=self.get_processed_semantic_features())
            out["render"].retain_grad()
            self.last_render = out["render"]
            return out

    module = Module()
    use_hip_smoothing(module, generator=torch.Generator().manual_seed(1))
    assert use_hip_loss(module) is module
    return module.train()


@pytest.mark.parametrize("scale_aware_dim", [-1, 8])
def test_one_training_step_matches_the_oracle(scale_aware_dim):
    from fakes import FakeCamera
    from oracle import gsplat_oracle as O
    masks, scales = SG.random_masks(20, *MASK_HW, seed=20)
    module = _module(scale_aware_dim, scales)
    cam = FakeCamera(O.synthetic_camera(W, H, 260.0), DEV)
    torch.manual_seed(7)
    semantic = (torch.from_numpy(masks).to(DEV).bool(), torch.from_numpy(scales).to(DEV))
    rendered, loss, cosine_pos, cosine_neg, norm = module.forward_with_loss_calculation(cam, None, semantic)
    assert rendered is module.last_render and tuple(rendered.shape) == (C, H, W)      # the renderer's map, not a resampled one
    loss.backward(retain_graph=True)
    step = module.hip_segany_step
    S = step.pixel_index.numel()
    assert 40 <= S <= 400 and step.upper.dtype == torch.bool and bool(step.upper[0])

    # what the step formed, against the oracle fed with the same draws
    pixel_index = step.pixel_index.cpu().numpy()
    order = np.argsort(-scales, kind="stable")
    member, _ = SG.membership(masks, order, pixel_index)
    scale_index, upper = step.scale_index.cpu().numpy(), step.upper.cpu().numpy()
    _, labels, counts = SG.pair_labels(member, scale_index, upper)
    assert np.array_equal(step.labels.cpu().numpy(), labels) and np.array_equal(step.counts.cpu().numpy(), counts)
    _, cover, mean_size, mean_bound = SG.mask_stats(masks)
    assert (cover.reshape(-1)[pixel_index] > 0).all()
    a = step.a.cpu().numpy()
    _within(a, mean_size.reshape(-1)[pixel_index], mean_bound.reshape(-1)[pixel_index], "a")
    gates = step.gates.detach().cpu().numpy()
    map32 = rendered.detach().cpu().numpy()
    ref = SG.loss(map32, MASK_HW, pixel_index, gates, labels, counts, a, step.rand.cpu().numpy(), lock=step.selected.cpu().numpy())
    firm = ~ref["fragile"]
    assert np.array_equal(step.selected.cpu().numpy()[firm], ref["own"][firm]) and ref["fragile"].sum() <= 1e-3 * S * (S - 1) / 2 + 2

    # the norm regulariser, in float64
    r64 = torch.from_numpy(map32.astype(np.float64)).requires_grad_(True)
    mean_norm = r64.norm(dim=0, p=2).mean()
    reg = module.rfn * (1 - mean_norm) ** 2
    reg.backward()
    Ns = gates.shape[0]
    r_corr = C + 8 + 8 * ref["kappa"]
    _within(float(loss.detach()), ref["loss"] + float(reg.detach()), EPS * ((r_corr + Ns + 12) * ref["loss_abs"] + 16 * (1 + float(reg.detach()))), "loss")
    _within(float(cosine_pos), ref["cosine_pos"], EPS * (r_corr + Ns + 12), "cosine_pos")
    _within(float(cosine_neg), ref["cosine_neg"], EPS * (r_corr + Ns + 12), "cosine_neg")
    _within(float(norm.detach()), float(mean_norm.detach()), 1e-5, "rendered_feature_norm")

    r_grad = S + 2 * C + Ns + 8 * ref["kappa"] + 16
    reg_grad = r64.grad.numpy()
    bound = EPS * ((r_grad + 4 + ref["texel_sharing"]) * ref["v_rendered_abs"] + 16 * np.abs(reg_grad)) + ref["v_rendered_fragile"] + 1e-12
    _within(rendered.grad.cpu().numpy(), ref["v_rendered"] + reg_grad, bound, "v_rendered")

    features = module.gaussian_semantic_features
    got = features.grad.cpu().double().numpy()
    pulled, = torch.autograd.grad(rendered, features, grad_outputs=torch.from_numpy((ref["v_rendered"] + reg_grad).astype(np.float32)).to(DEV))
    want = pulled.cpu().double().numpy()
    rms = np.sqrt(np.mean(want * want))
    assert rms > 0 and (np.abs(got - want) <= 1e-4 * (np.abs(want) + rms)).all(), "gaussian_semantic_features' gradient"

    linear = module.scale_gate[0]
    if scale_aware_dim <= 0:
        s = step.sampled_scales.cpu().double().numpy().reshape(-1)
        g64 = 1 / (1 + np.exp(-(s[:, None] * linear.weight.detach().cpu().double().numpy()[:, 0][None] + linear.bias.detach().cpu().double().numpy()[None])))
        _within(gates, g64, 8 * EPS, "gates")
        slope = g64 * (1 - g64)
        tolerance = (EPS * (r_grad + -(-S // 64) + 7 + 8 + Ns) * ref["v_gates_abs"] + ref["v_gates_fragile"]) * slope
        _within(linear.weight.grad.cpu().numpy()[:, 0], (ref["v_gates"] * slope * s[:, None]).sum(axis=0), (tolerance * np.abs(s)[:, None]).sum(axis=0), "Linear.weight")
        _within(linear.bias.grad.cpu().numpy(), (ref["v_gates"] * slope).sum(axis=0), tolerance.sum(axis=0), "Linear.bias")
        assert np.abs(linear.weight.grad.cpu().numpy()).max() > 0
    else:
        assert linear.weight.grad is None and set(np.unique(gates)) <= {0.0, 1.0} and gates.sum(axis=1).min() >= 24


def test_mask_preprocess_returns_the_reference_tuple():
    masks, scales = SG.random_masks(20, *MASK_HW, seed=20)
    module = _module(-1, scales)
    torch.manual_seed(7)
    sampled_ray, weight, gt_corrs, sampled_scales = module.mask_preprocess(torch.from_numpy(masks).to(DEV), torch.from_numpy(scales).to(DEV))
    S = int(sampled_ray.sum())
    assert sampled_ray.dtype == torch.bool and tuple(sampled_ray.shape) == MASK_HW
    assert tuple(weight.shape) == (S, S) and tuple(gt_corrs.shape) == (10, S, S) and tuple(sampled_scales.shape) == (10,)
    step = module.hip_segany_step
    assert np.array_equal(weight.cpu().numpy(), SG.pair_weight(step.a.cpu().numpy()), equal_nan=True)
    assert np.array_equal(gt_corrs.cpu().numpy() != 0, SG.unpack_labels(step.labels.cpu().numpy(), 10))

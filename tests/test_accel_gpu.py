"""The fused Inria call's two switches on the GPU (GSPL_INRIA_ANTIALIAS, GSPL_INRIA_INVDEPTH), `SparseGaussianAdam` and the
`HipTaming3DGSRenderer` plugin: the fp64 oracle of tests/accel_oracle.py, bit-equality with the existing paths, a short training run."""
import math

import numpy as np
import pytest
import torch

from oracle import gsplat_oracle as O
import accel_oracle as A

pytestmark = pytest.mark.gpu

W, H = 160, 112
EPS_IN = 4 * 2.0 ** -24      # the two sides composite per-splat inputs that differ by a few fp32 ulps


def _scene(n=2000, seed=11, needles=40):
    means, scales, quats, opac, shs = O.synthetic_scene(n, seed=seed)
    scales = scales * 4
    scales[:needles, 1:] = 1e-6                  # needle-thin splats: det0 / det1 far below the 2.5e-5 floor
    cam = O.synthetic_camera(W, H, 150.0, 148.0)
    return (means, scales, quats, opac, shs), cam


def _settings(cam, bg, dev, antialiasing=False):
    from gspl_amd import ops
    return ops.AccelRasterizationSettings(image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=bg.to(dev),
                                          scale_modifier=1.0, viewmatrix=cam["world_to_camera"].to(dev), projmatrix=cam["full_projection"].to(dev),
                                          sh_degree=3, campos=cam["camera_center"].to(dev), antialiasing=antialiasing)


@pytest.fixture
def deterministic():
    """Bit-reproducible compositing gradients (per-splat rows added in list order, not by atomics in dispatch order)."""
    from gspl_amd import ops
    was = ops.set_deterministic(True)
    yield
    ops.set_deterministic(was)


def _grad_check(name, got, ref, rows):
    g, rf = got.detach().cpu().double().numpy(), ref.detach().numpy()
    rms = np.sqrt(np.mean(rf * rf)) + 1e-30
    rel = np.abs(g - rf) / (np.abs(rf) + rms)
    reach = np.broadcast_to(rows.reshape((-1,) + (1,) * (rf.ndim - 1)), rf.shape)
    assert np.mean(rel <= 1e-4) > 0.995, f"gradient parity {name}: worst {rel.max():.3e}"
    loose = int(((rel > 5e-4) & ~reach).sum())
    band = int(((rel > 1e-4) & (rel <= 5e-4) & ~reach).sum())
    assert loose == 0 and band <= max(2e-5 * rel.size, 1.0), f"gradient parity {name}: {loose} beyond 5e-4, {band} beyond 1e-4 in unreachable rows"
    assert float(rel.max()) <= 0.05, f"gradient parity {name}: worst element {float(rel.max()):.3e}"


@pytest.mark.parametrize("aa,invd", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("colour", ["shs", "shs_rest", "colors_precomp"])
def test_accel_against_fp64_oracle(aa, invd, raw, colour):
    from gspl_amd import ops
    dev = torch.device("cuda:0")
    (means, scales, quats, opac, shs), cam = _scene(seed=11 + 3 * raw + (colour == "shs_rest"))
    bg = torch.tensor([0.3, 0.1, 0.6])
    cp = torch.rand(means.shape[0], 3, generator=torch.Generator().manual_seed(5))
    if raw:      # the model's raw parameters: log-scales, unnormalised quaternions, logits
        s_in, q_in, o_in = scales.log(), quats * 1.7, torch.logit(opac.clamp(1e-4, 1 - 1e-4))
    else:
        s_in, q_in, o_in = scales, quats, opac
    c_in = cp if colour == "colors_precomp" else shs
    leaves = [t.to(dev).requires_grad_(True) for t in (means, s_in, q_in, o_in, c_in)]
    m, s, q, o, c = leaves
    screen = torch.zeros_like(m, requires_grad=True)
    kw = dict(colors_precomp=c) if colour == "colors_precomp" else (dict(shs=c[:, :1], shs_rest=c[:, 1:]) if colour == "shs_rest" else dict(shs=c))
    ops.KEEP_LAST_RASTER = True
    try:
        img, radii, inv = ops.rasterize_inria_accel(_settings(cam, bg, dev), m, screen, o, scales=s, rotations=q, raw_parameters=raw,
                                                    antialiasing=aa, inverse_depth=invd, **kw)
        last_opac = ops.LAST_RASTER["opacities"].detach().cpu().clone()
    finally:
        ops.KEEP_LAST_RASTER = False
    gen = torch.Generator().manual_seed(9)
    w_img = torch.rand(3, H, W, generator=gen).double()
    w_inv = torch.rand(1, H, W, generator=gen).double()
    loss = (img * w_img.float().to(dev)).sum() + ((inv * w_inv.float().to(dev)).sum() if invd else 0.0)
    loss.backward()
    torch.cuda.synchronize()

    dl = [t.double().requires_grad_(True) for t in (means, s_in, q_in, o_in, c_in)]
    md, sd, qd, od, cd = dl
    if raw:
        sd_a, qd_a, od_a = sd.exp(), torch.nn.functional.normalize(qd, dim=-1), torch.sigmoid(od)
    else:
        sd_a, qd_a, od_a = sd, qd, od
    r = A.render_inria_accel(md, sd_a, qd_a, od_a, None if colour == "colors_precomp" else cd, 3, cam["world_to_camera"].double(),
                             cam["full_projection"].double(), cam["camera_center"].double(), cam["tanfovx"], cam["tanfovy"], W, H, bg.double(),
                             antialias=aa, colors_precomp=cd if colour == "colors_precomp" else None)
    ref_loss = (r["render"] * w_img).sum() + ((r["inverse_depth"] * w_inv).sum() if invd else 0.0)
    ref_loss.backward()
    assert np.array_equal(radii.cpu().numpy(), r["radii"].numpy())
    xy, con, feats, op = r["xy"].detach(), r["conics"].detach(), r["features"].detach(), r["opacities"].detach()
    _, _, _, frag = O.composite_fwd(O.MODE_INRIA, xy, con, feats, op, None, W, H, r["offsets"], r["flatten_ids"], input_eps=EPS_IN)
    frag = O.fragile_order(O.MODE_INRIA, xy, con, op, r["depths"].detach(), W, H, r["offsets"], r["flatten_ids"], fragile_px=frag, tol_rel=EPS_IN)
    firm = frag == 0
    got = [img.detach().cpu().double()] + ([inv.detach().cpu().double()] if invd else [])
    want = [r["render"].detach()] + ([r["inverse_depth"].detach()] if invd else [])
    for a, b in zip(got, want):
        diff = (a - b).abs().numpy()
        assert float(diff[np.broadcast_to(firm, diff.shape)].max()) <= 1e-5
    if aa:
        # the needles reach the floor — in the oracle and in the KERNEL's effective opacities (state->opacities)
        vis = r["mask"][:40]
        assert bool(vis.any()), "no needle is visible"
        comp = A.compensation(md.detach(), sd_a.detach(), 1.0, qd_a.detach(), cam["world_to_camera"].double(), cam["tanfovx"], cam["tanfovy"], W, H)
        assert bool((comp[:40][vis] <= 2.5e-5 ** 0.5 + 1e-12).all())
        eff = last_opac.double()[:40][vis]
        want = r["opacities"].detach()[:40][vis]
        assert torch.allclose(eff, want, rtol=1e-5, atol=1e-9), (eff[:4], want[:4])
    rows = O.fragile_splats(O.MODE_INRIA, xy, con, op, W, H, r["offsets"], r["flatten_ids"], frag, input_eps=EPS_IN)
    for got_t, ref_t, name in zip(leaves, dl, ("means", "scales", "rotations", "opacities", "colour")):
        _grad_check(name, got_t.grad, ref_t.grad, rows)


def test_default_path_is_the_existing_rasterizer_bit_for_bit(deterministic):
    from gspl_amd import ops
    dev = torch.device("cuda:0")
    (means, scales, quats, opac, shs), cam = _scene(seed=21)
    bg = torch.tensor([0.2, 0.5, 0.1])
    outs = []
    for which in ("existing", "accel_off", "accel_invd"):
        leaves = [t.to(dev).requires_grad_(True) for t in (means, scales, quats, opac, shs)]
        m, s, q, o, c = leaves
        screen = torch.zeros_like(m, requires_grad=True)
        st = _settings(cam, bg, dev)
        if which == "existing":
            img, radii = ops.GaussianRasterizer(ops.GaussianRasterizationSettings(*st[:-1]))(m, screen, o, shs=c[:, :1], shs_rest=c[:, 1:],
                                                                                              scales=s, rotations=q)
        else:
            img, radii, inv = ops.rasterize_inria_accel(st, m, screen, o, c[:, :1], scales=s, rotations=q, shs_rest=c[:, 1:],
                                                        inverse_depth=(which == "accel_invd"))
        (img * torch.linspace(0, 1, W, device=dev)).sum().backward()
        outs.append([img.detach(), radii] + [t.grad for t in leaves] + [screen.grad])
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1])      # rgb unchanged by the 4th channel
    # ... and with anti-aliasing on, too
    imgs = []
    for invd in (False, True):
        m, s, q, o, c = [t.to(dev) for t in (means, scales, quats, opac, shs)]
        with torch.no_grad():
            img, _, _ = ops.rasterize_inria_accel(_settings(cam, bg, dev), m, torch.zeros_like(m), o, c, scales=s, rotations=q,
                                                  antialiasing=True, inverse_depth=invd)
        imgs.append(img)
    assert torch.equal(imgs[0], imgs[1])


def test_sparse_gaussian_adam_is_selective_adam():
    from gspl_amd import optimizers
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)
    p0 = torch.randn(5000, 3, device=dev, generator=g)
    pa, pb = torch.nn.Parameter(p0.clone()), torch.nn.Parameter(p0.clone())
    a = optimizers.SparseGaussianAdam([{"params": [pa], "name": "xyz"}], lr=1e-2, eps=1e-15)
    b = optimizers.SelectiveAdam([{"params": [pb], "name": "xyz"}], lr=1e-2, eps=1e-15, betas=(0.9, 0.999))
    for step in range(5):
        grad = torch.randn(5000, 3, device=dev, generator=g)
        vis = torch.rand(5000, device=dev, generator=g) > 0.4
        pa.grad, pb.grad = grad.clone(), grad.clone()
        before = pa.detach().clone()
        a.step(vis, 5000)
        b.step(vis)
        assert torch.equal(pa, pb)
        assert torch.equal(pa[~vis], before[~vis])      # invisible rows untouched
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(a.state[pa][k], b.state[pb][k])
    # loads a torch.optim.Adam state dict
    pc = torch.nn.Parameter(p0.clone())
    ref = torch.optim.Adam([{"params": [pc], "name": "xyz"}], lr=1e-2, eps=1e-15)
    pc.grad = torch.randn_like(pc)
    ref.step()
    pd = torch.nn.Parameter(pc.detach().clone())
    c = optimizers.SparseGaussianAdam([{"params": [pd], "name": "xyz"}], lr=1e-2, eps=1e-15)
    c.load_state_dict(ref.state_dict())
    assert torch.equal(c.state[pd]["exp_avg"], ref.state[pc]["exp_avg"])
    pd.grad = torch.randn_like(pd)
    c.step(torch.ones(5000, dtype=torch.bool, device=dev), 5000)
    assert bool(torch.isfinite(pd).all())


def test_sparse_gaussian_adam_survives_density_surgery():
    """The density controller's state surgery (prune: index the moments; densify: cat zeros), as for torch.optim.Adam."""
    from gspl_amd import optimizers
    dev = torch.device("cuda:0")
    p = torch.nn.Parameter(torch.randn(1000, 3, device=dev))
    opt = optimizers.SparseGaussianAdam([{"params": [p], "name": "xyz"}], lr=1e-2, eps=1e-15)
    p.grad = torch.randn_like(p)
    opt.step(torch.ones(1000, dtype=torch.bool, device=dev), 1000)
    keep = torch.arange(1000, device=dev) % 3 != 0
    group = opt.param_groups[0]
    st = opt.state.pop(group["params"][0])
    st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"][keep], st["exp_avg_sq"][keep]
    new = torch.nn.Parameter(torch.cat([p.detach()[keep], torch.randn(50, 3, device=dev)]))
    st["exp_avg"] = torch.cat([st["exp_avg"], torch.zeros(50, 3, device=dev)])
    st["exp_avg_sq"] = torch.cat([st["exp_avg_sq"], torch.zeros(50, 3, device=dev)])
    group["params"][0] = new
    opt.state[new] = st
    n = new.shape[0]
    new.grad = torch.randn_like(new)
    vis = torch.rand(n, device=dev) > 0.5
    before = new.detach().clone()
    opt.step(vis, n)
    assert bool(torch.isfinite(new).all()) and torch.equal(new[~vis], before[~vis]) and not torch.equal(new[vis], before[vis])


def test_fuse_into_backward_falls_back_with_antialiasing(deterministic):
    from gspl_amd import ops, optimizers
    dev = torch.device("cuda:0")
    (means, scales, quats, opac, shs), cam = _scene(seed=31)
    results = []
    for fuse in (False, True):
        params = [torch.nn.Parameter(t.to(dev).clone()) for t in (means, scales, quats, opac, shs[:, :1].contiguous(), shs[:, 1:].contiguous())]
        names = ["xyz", "scaling", "rotation", "opacity", "f_dc", "f_rest"]
        opt = optimizers.FusedAdam([{"params": [p], "name": nm} for p, nm in zip(params, names)], lr=1e-3, fuse_into_backward=fuse)
        try:
            for _ in range(3):
                m, s, q, o, dc, rest = params
                img, radii, inv = ops.rasterize_inria_accel(_settings(cam, torch.zeros(3), dev, antialiasing=True), m, torch.zeros_like(m),
                                                            o, dc, scales=s, rotations=q, shs_rest=rest, antialiasing=True, inverse_depth=False)
                (img - 0.3).abs().mean().backward()
                assert params[0].grad is not None      # the backward wrote gradients: no update inside it
                opt.step()
                opt.zero_grad(set_to_none=True)
        finally:
            opt.fuse_into_backward = False
        results.append([p.detach().clone() for p in params])
    for a, b in zip(*results):
        assert torch.equal(a, b)


class _RawModel(torch.nn.Module):
    """Stores RAW parameters (log-scales, quaternions, logits) and declares its activations (renderer.model_raw_parameters)."""
    fused_activations = {"scales": "exp", "rotations": "normalize", "opacities": "sigmoid"}

    def __init__(self, means, scales, quats, opac, shs):
        super().__init__()
        P = torch.nn.Parameter
        self.means, self.scales_, self.rotations_ = P(means), P(scales.log()), P(quats)
        self.opacities_ = P(torch.logit(opac.clamp(1e-4, 1 - 1e-4)))
        self.shs_dc, self.shs_rest = P(shs[:, :1].contiguous()), P(shs[:, 1:].contiguous())
        self.active_sh_degree, self.is_pre_activated = 3, False

    get_xyz = property(lambda s: s.means)
    get_scaling = property(lambda s: torch.exp(s.scales_))
    get_rotation = property(lambda s: torch.nn.functional.normalize(s.rotations_))
    get_opacity = property(lambda s: torch.sigmoid(s.opacities_))

    def get_property(self, name):
        return {"scales": self.scales_, "rotations": self.rotations_, "opacities": self.opacities_}[name]

    def get_shs_dc(self):
        return self.shs_dc

    def get_shs_rest(self):
        return self.shs_rest


def test_taming_renderer_trains_with_sparse_adam():
    from fakes import FakeCamera
    from gspl_amd import ops, optimizers
    from gspl_amd.renderers import HipTaming3DGSRenderer
    dev = torch.device("cuda:0")
    (means, scales, quats, opac, shs), cam = _scene(n=3000, seed=41, needles=0)
    camera = FakeCamera(cam, dev)
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        target_img, _, target_inv = ops.rasterize_inria_accel(_settings(cam, bg, dev, True), means.to(dev), torch.zeros(3000, 3, device=dev),
                                                              opac.to(dev), shs.to(dev), scales=scales.to(dev), rotations=quats.to(dev),
                                                              antialiasing=True, inverse_depth=True)
    gen = torch.Generator().manual_seed(2)
    model = _RawModel(means + 0.05 * torch.randn(means.shape, generator=gen), scales * 1.3, quats, opac * 0.7 + 0.05,
                      shs + 0.1 * torch.randn(shs.shape, generator=gen)).to(dev)
    params = [model.means, model.scales_, model.rotations_, model.opacities_, model.shs_dc, model.shs_rest]
    from gspl_amd.renderers.renderer import model_raw_parameters
    assert model_raw_parameters(model) is not None      # the plugin hands the kernels the raw parameters (RAW + AA backward)
    opt = optimizers.HipSparseGaussianAdam().instantiate([{"params": [p], "name": str(i)} for i, p in enumerate(params)], 2e-3, eps=1e-15)
    renderer = HipTaming3DGSRenderer(anti_aliased=True)
    misses0 = ops.SPECULATION["misses"]
    losses = []
    for step in range(200):
        out = renderer(camera, model, bg, render_types=["rgb", "inverse_depth"])
        loss = (out["render"] - target_img).abs().mean() + 0.1 * (out["inverse_depth"] - target_inv).abs().mean()
        loss.backward()
        opt.on_after_backward(out, None, model, step, None)
        opt.step()
        opt.zero_grad(set_to_none=True)
        losses.append(float(loss))
    assert all(math.isfinite(v) for v in losses)
    assert all(bool(torch.isfinite(p).all()) for p in params)
    assert np.mean(losses[-10:]) < 0.8 * np.mean(losses[:10]), (losses[:3], losses[-3:])
    assert ops.SPECULATION["misses"] == misses0

"""The 3DGS-MCMC kernels (csrc/mcmc.hip, include/gspl_hip.h section 13) and the `gspl_amd.mcmc` controller on the GPU, against the fp64
oracle of tests/mcmc_oracle.py: relocation over every n, the noise step with given and in-kernel normals (the Philox words pinned bit
for bit), the regulariser, guard bands, degenerate inputs, one relocation event of the plugin, and a short MCMC training run."""
import ctypes
import math

import numpy as np
import pytest
import torch

import gspl_amd  # noqa: F401
from gspl_amd import _lib as L
from gspl_amd import ops, optimizers, synthetic
from gspl_amd.ops import mcmc as M

import mcmc_oracle as MO

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def dev():
    return torch.device("cuda:0")


def _binoms(n_max=51):
    return torch.tensor(MO.binoms(n_max), dtype=torch.float32, device=dev())


def _relocation_inputs():
    ns = list(range(0, 54))                                       # 0 and 52, 53 are clamped to 1 and 51
    op = np.concatenate([np.geomspace(0.005, 0.5, 24), 1 - np.geomspace(0.5, 2.0 ** -23, 24)]).astype(np.float32)
    n = np.repeat(np.array(ns, dtype=np.int32), op.size)
    o = np.tile(op, len(ns))
    rng = np.random.default_rng(3)
    s = (10.0 ** rng.uniform(-3, 3, size=(o.size, 3))).astype(np.float32)
    return o, s, n


def test_relocation_against_the_oracle_for_every_n():
    o, s, n = _relocation_inputs()
    ratios = torch.tensor(n, device=dev()).to(torch.int64)
    before = ratios.clone()
    new_o, new_s = ops.compute_relocation(torch.tensor(o, device=dev()), torch.tensor(s, device=dev()), ratios, _binoms())
    assert torch.equal(ratios, before), "the caller's ratios were modified"
    ro, rs, kappa = MO.relocation(o, s, n, 51)
    nn_ = np.clip(n, 1, 51)
    got_o, got_s = new_o.cpu().double().numpy(), new_s.cpu().double().numpy()
    err_o = np.abs(got_o - ro) / ro
    assert err_o.max() <= 16 * U, f"new opacity: worst relative error {err_o.max():.3e}"
    # new_scales = (o / denom) s: recursive fp32 summation of n(n+1)/2 terms, each carrying up to 3(k+1) rounding errors of x^(k+1)
    c = nn_ * (nn_ + 1) / 2 + 3 * nn_ + 16
    err_s = (np.abs(got_s - rs) / np.abs(rs)).max(axis=1)
    bound = c * kappa * U
    assert np.all(err_s <= bound), f"new scales: rows beyond c kappa 2^-24: {np.argwhere(err_s > bound)[:5].ravel()}"
    # the bound above is loose where kappa is large (n = 51, o near 1: it allows ~2.6); what the fp32 sum does there in fact: the
    # denominator (~2) keeps its sign and its first three digits — an fp32 simulation of the written order over this grid errs by
    # 6.3e-4 at most — so every new scale is finite and positive (its log, the model's raw scale, is defined)
    assert np.all(np.isfinite(got_s)) and np.all(got_s > 0)
    assert err_s.max() <= 5e-3, f"new scales: worst relative error {err_s.max():.3e}"
    well = kappa < 10
    assert well.sum() > 1000 and err_s[well].max() <= 1e-5, f"kappa < 10 rows: worst {err_s[well].max():.3e}"
    # closed forms: n = 1 is the identity, n = 2 has denom 2x - x^2 / sqrt(2)
    one = nn_ == 1
    assert np.array_equal(got_o[one], o[one].astype(np.float64)) and np.array_equal(got_s[one], s[one].astype(np.float64))


def test_relocation_accepts_int32_and_degenerate_sizes():
    b = _binoms()
    o = torch.tensor([0.4], device=dev())
    s = torch.tensor([[1.0, 2.0, 3.0]], device=dev())
    for dt in (torch.int32, torch.int64, torch.int16, torch.uint8):
        a, c = ops.compute_relocation(o, s, torch.tensor([2], device=dev(), dtype=dt), b)
        x = float(a)
        assert abs(x - (1 - math.sqrt(0.6))) < 1e-6
        assert abs(float(c[0, 0]) - 0.4 / (2 * x - x * x / math.sqrt(2))) < 1e-5
    a, c = ops.compute_relocation(torch.empty(0, device=dev()), torch.empty(0, 3, device=dev()), torch.empty(0, dtype=torch.int32, device=dev()), b)
    assert a.shape == (0,) and c.shape == (0, 3)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.compute_relocation(o, torch.ones(1, 6, device=dev())[:, ::2], torch.tensor([2], device=dev()), b)


def _noise_scene(n=20000, seed=5):
    means, scales, quats, opac, _ = synthetic.scene(n, seed=seed)
    opac = torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 0.999 + 0.0005     # the steep sigmoid's whole range
    return means.float(), scales.float(), quats.float(), opac.float()


@pytest.mark.parametrize("raw", [False, True])
def test_perturbation_with_given_noise_against_the_oracle(raw):
    means, scales, quats, opac = _noise_scene()
    if raw:
        s_in, q_in, o_in = scales.log(), quats * 1.7, torch.logit(opac)
    else:
        s_in, q_in, o_in = scales, torch.nn.functional.normalize(quats), opac
    eps = torch.randn(means.shape, generator=torch.Generator().manual_seed(9))
    coeff = 5e5 * 1.6e-4
    ref = MO.perturb(means.numpy(), s_in.numpy(), q_in.numpy(), o_in.numpy(), eps.numpy(), coeff, raw)
    m = means.to(dev())
    ops.perturb_means_(m, s_in.to(dev()), q_in.to(dev()), o_in.to(dev()).reshape(-1, 1), raw=raw, noise_scale=coeff, noise=eps.to(dev()))
    got = m.cpu().double().numpy()
    step = np.abs(ref - means.numpy().astype(np.float64))
    err = np.abs(got - ref)
    tol = 2e-6 * np.abs(ref) + 1e-5 * step.max(axis=1, keepdims=True) + 1e-30
    assert np.all(err <= tol), f"worst error {err.max():.3e}; over tolerance: {(err > tol).sum()}"


def test_raw_and_activated_paths_agree():
    means, scales, quats, opac = _noise_scene(4099)
    eps = torch.randn(means.shape, generator=torch.Generator().manual_seed(2)).to(dev())
    a, b = means.to(dev()), means.to(dev())
    ops.perturb_means_(a, scales.log().to(dev()), quats.to(dev()), torch.logit(opac).to(dev()), raw=True, noise_scale=80.0, noise=eps)
    ops.perturb_means_(b, scales.to(dev()), torch.nn.functional.normalize(quats).to(dev()), opac.to(dev()), raw=False, noise_scale=80.0, noise=eps)
    d = (a - means.to(dev())).abs().max().item()
    assert d > 0 and torch.allclose(a, b, rtol=1e-5, atol=1e-5 * d)


def test_in_kernel_philox_is_pinned_bit_for_bit():
    seed, offset = 0x1234_5678_9ABC_DEF1, 0x0000_0003_0000_0010
    n = 100003
    normals, words = ops.mcmc_randn(n, seed, offset, dev(), bits=True)
    ref_bits = MO.mcmc_bits(n, seed, offset)
    assert np.array_equal(words.cpu().numpy().view(np.uint32), ref_bits)
    ref = MO.box_muller(ref_bits)
    assert np.abs(normals.cpu().double().numpy() - ref).max() <= 4e-6
    # the noise kernel draws the same normals: in-kernel eps == supplied eps, bit for bit
    means, scales, quats, opac = _noise_scene(n)
    a, b = means.to(dev()), means.to(dev())
    args = (scales.to(dev()), torch.nn.functional.normalize(quats).to(dev()), opac.to(dev()))
    g = torch.Generator(device=dev())
    g.manual_seed(seed)
    g.set_offset(offset)
    ops.perturb_means_(a, *args, raw=False, noise_scale=80.0, generator=g)
    assert g.get_offset() == offset + M.OFFSET_STEP
    ops.perturb_means_(b, *args, raw=False, noise_scale=80.0, noise=normals)
    assert torch.equal(a, b)


def test_noise_is_reproducible_and_never_repeats():
    means, scales, quats, opac = _noise_scene(5000)
    args = (scales.to(dev()), torch.nn.functional.normalize(quats).to(dev()), opac.to(dev()))
    outs = []
    for _ in range(2):
        torch.manual_seed(123)
        gen = torch.cuda.default_generators[0]
        off0 = gen.get_offset()
        m1 = means.to(dev())
        ops.perturb_means_(m1, *args, raw=False, noise_scale=80.0)
        m2 = m1.clone()
        ops.perturb_means_(m2, *args, raw=False, noise_scale=80.0)
        assert gen.get_offset() == off0 + 2 * M.OFFSET_STEP
        outs.append((m1, m2))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    d1, d2 = outs[0][0] - means.to(dev()), outs[0][1] - outs[0][0]
    assert not torch.equal(d1, d2)


def test_philox_normals_are_standard_normal():
    n = 4 * 1024 * 1024 // 3 + 1          # 4 M draws
    z = ops.mcmc_randn(n, 42, 8, dev()).double()
    N = z.shape[0]
    mean, cov = z.mean(0), torch.cov(z.t())
    se_mean, se_var, se_cov = 1 / math.sqrt(N), math.sqrt(2 / N), 1 / math.sqrt(N)
    assert (mean.abs() <= 5 * se_mean).all(), mean
    assert ((cov.diagonal() - 1).abs() <= 5 * se_var).all(), cov
    off = cov - torch.diag(cov.diagonal())
    assert (off.abs() <= 5 * se_cov).all(), cov


@pytest.mark.parametrize("raw", [False, True])
def test_regulariser_against_the_oracle_and_bit_reproducible(raw):
    n = 300007
    g = torch.Generator().manual_seed(4)
    o = (torch.randn(n, 1, generator=g) * 2) if raw else torch.rand(n, 1, generator=g)
    s = (torch.randn(n, 3, generator=g) - 4) if raw else torch.rand(n, 3, generator=g) * 0.1
    od, sd = o.to(dev()).requires_grad_(True), s.to(dev()).requires_grad_(True)
    lo, ls = ops.mcmc_regularization(od, sd, 0.01, 0.02, raw=raw)
    (3.0 * lo + 5.0 * ls).backward()
    ro, rs = MO.reg_fwd(o.numpy(), s.numpy(), 0.01, 0.02, raw)
    assert abs(lo.item() - ro) <= 1e-5 * ro and abs(ls.item() - rs) <= 1e-5 * rs
    vo, vs = MO.reg_bwd(o.numpy(), s.numpy(), 0.01, 0.02, raw, 3.0, 5.0)
    assert np.allclose(od.grad.cpu().numpy(), vo, rtol=1e-5, atol=1e-12)
    assert np.allclose(sd.grad.cpu().numpy(), vs, rtol=1e-5, atol=1e-12)
    again = [ops.mcmc_regularization(od.detach(), sd.detach(), 0.01, 0.02, raw=raw) for _ in range(5)]
    for a, b in again:
        assert a.item() == lo.item() and b.item() == ls.item()


def _guarded(n, dtype=torch.float32, band=64):
    """A tensor of n elements in the middle of a buffer pre-filled with 0xFF, and a check that both bands are intact."""
    buf = torch.full((n + 2 * band,), -1, dtype=torch.int32, device=dev())
    view = buf[band:band + n].view(dtype)
    return view, lambda: bool((buf[:band] == -1).all()) and bool((buf[band + n:] == -1).all())


def test_guard_bands_of_every_output():
    m = 1001
    o, s, n = _relocation_inputs()
    o, s, n = (torch.tensor(t[:m], device=dev()) for t in (o, s, n))
    no, ok1 = _guarded(m)
    ns, ok2 = _guarded(3 * m)
    L.call("gspl_mcmc_relocation", m, 51, L.ptr(o), L.ptr(s), L.ptr(n), L.ptr(_binoms()), L.ptr(no), L.ptr(ns), L.stream())
    words, ok3 = _guarded(4 * m, torch.int32)
    normals, ok4 = _guarded(3 * m)
    L.call("gspl_mcmc_randn", m, 5, 4, L.ptr(words), L.ptr(normals), L.stream())
    means, ok5 = _guarded(3 * m)
    means.copy_(torch.randn(3 * m, device=dev()))
    q = torch.nn.functional.normalize(torch.randn(m, 4, device=dev()))
    sc = torch.rand(m, 3, device=dev()) * 0.1
    L.call("gspl_mcmc_perturb_means", m, 0, L.ptr(means), L.ptr(sc), L.ptr(q), L.ptr(no), None, ctypes.c_float(1.0), 1, 0, L.stream())
    sc_raw = sc.log()
    L.call("gspl_mcmc_perturb_means", m, 1, L.ptr(means), L.ptr(sc_raw), L.ptr(q), L.ptr(no), L.ptr(normals), ctypes.c_float(1.0), 0, 0, L.stream())
    G = L.lib().gspl_mcmc_reg_partials(m)
    part, ok6 = _guarded(2 * G)
    out, ok7 = _guarded(2)
    L.call("gspl_mcmc_reg_fwd", m, 1, L.ptr(no), L.ptr(sc), ctypes.c_float(0.1), ctypes.c_float(0.1), L.ptr(part), L.ptr(out), L.stream())
    vo, ok8 = _guarded(m)
    vs, ok9 = _guarded(3 * m)
    go = torch.ones(2, device=dev())
    L.call("gspl_mcmc_reg_bwd", m, 1, L.ptr(no), L.ptr(sc), ctypes.c_float(0.1), ctypes.c_float(0.1), L.ptr(go), L.ptr(vo), L.ptr(vs), L.stream())
    torch.cuda.synchronize()
    assert all(f() for f in (ok1, ok2, ok3, ok4, ok5, ok6, ok7, ok8, ok9))
    assert torch.isfinite(means).all() and torch.isfinite(out).all() and torch.isfinite(vs).all()


def test_degenerate_inputs():
    z = torch.empty(0, 3, device=dev())
    assert ops.perturb_means_(z, z.clone(), torch.empty(0, 4, device=dev()), torch.empty(0, device=dev()), raw=True, noise_scale=1.0) is z
    a, b = ops.mcmc_regularization(torch.empty(0, 1, device=dev()), z, 0.1, 0.1, raw=True)
    assert a.item() == 0 and b.item() == 0
    one = torch.zeros(1, 3, device=dev())
    torch.manual_seed(0)
    ops.perturb_means_(one, torch.full((1, 3), -1.0, device=dev()), torch.tensor([[1.0, 0, 0, 0]], device=dev()),
                       torch.tensor([-8.0], device=dev()), raw=True, noise_scale=1.0)
    assert torch.isfinite(one).all() and one.abs().sum() > 0
    wide = torch.zeros(8, 6, device=dev())
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.perturb_means_(wide[:, :3], torch.zeros(8, 3, device=dev()), torch.zeros(8, 4, device=dev()), torch.zeros(8, device=dev()),
                           raw=True, noise_scale=1.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.perturb_means_(torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 4), torch.zeros(2), raw=True, noise_scale=1.0)


def test_noise_step_at_one_million_against_the_oracle_on_sampled_rows():
    n = 1_000_000
    means, scales, quats, opac = _noise_scene(n, seed=11)
    raw = (scales.log().to(dev()), quats.to(dev()), torch.logit(opac).to(dev()).reshape(-1, 1))
    m = means.to(dev())
    seed, offset = 77, 1024
    g = torch.Generator(device=dev())
    g.manual_seed(seed)
    g.set_offset(offset)
    ops.perturb_means_(m, *raw, raw=True, noise_scale=80.0, generator=g)
    rows = np.random.default_rng(0).choice(n, 4000, replace=False)
    eps = np.concatenate([MO.box_muller(MO.mcmc_bits(1, seed, offset, first=int(r))) for r in rows])
    ref = MO.perturb(means.numpy()[rows], raw[0].cpu().numpy()[rows], raw[1].cpu().numpy()[rows], raw[2].cpu().numpy()[rows], eps, 80.0, True)
    got = m.cpu().double().numpy()[rows]
    step = np.abs(ref - means.numpy()[rows].astype(np.float64)).max(axis=1, keepdims=True)
    assert np.all(np.abs(got - ref) <= 2e-6 * np.abs(ref) + 1e-5 * step + 1e-30)


# ---- the controller on the GPU --------------------------------------------------------------------------------------------------------
import bench_loop  # noqa: E402
from gspl_amd import mcmc as plugin  # noqa: E402


class _Model(bench_loop.RawGaussians):
    """bench_loop's raw-parameter model plus what the MCMC controller touches of the reference's model: settable properties and the
    inverse activations (vanilla_gaussian.py:348-355)."""
    properties = property(lambda s: s.gaussians, lambda s, v: setattr(s, "gaussians", dict(v)))

    def opacity_inverse_activation(self, o):
        return torch.log(o / (1 - o))

    def scale_inverse_activation(self, s):
        return torch.log(s)


class _Module:
    def __init__(self, model, optimizers):
        self.device, self.gaussian_model, self.gaussian_optimizers = dev(), model, optimizers
        self.on_train_batch_end_hooks = []

    def is_final_step(self, step=None):
        return False


def _oracle_relocation(o, s, n, binoms):
    ro, rs, _ = MO.relocation(o.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy(), binoms.shape[0])
    return torch.tensor(ro, dtype=torch.float32, device=o.device), torch.tensor(rs, dtype=torch.float32, device=o.device)


def _scene_model(n=6000, seed=3):
    means, scales, quats, opac, shs = synthetic.scene(n, seed=seed)
    opac = opac.clone()
    opac[::7] = 0.003                                     # dead ones to relocate
    return _Model(*(t.to(dev()) for t in (means, scales, quats, opac, shs)), active_sh_degree=3)


def _render_step(model, opts, cam, target):
    g = model.gaussians
    st = ops.GaussianRasterizationSettings(cam["height"], cam["width"], cam["tanfovx"], cam["tanfovy"], torch.zeros(3, device=dev()), 1.0,
                                           cam["world_to_camera"], cam["full_projection"], 3, cam["camera_center"])
    screen = torch.empty_like(g["means"]).requires_grad_(True)
    img, _ = ops.GaussianRasterizer(st)(g["means"], screen, g["opacities"], shs=g["shs_dc"], shs_rest=g["shs_rest"], scales=g["scales"],
                                        rotations=g["rotations"], raw_parameters=True)
    loss = (img - target).abs().mean()
    return loss


def _camera(W=192, H=128):
    c = synthetic.camera(W, H, 180.0)
    c = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in c.items()}
    c["width"], c["height"] = W, H
    return c


@pytest.mark.parametrize("fuse", [False, True])
def test_relocation_event_matches_the_torch_restated_math_and_clears_adam_rows(monkeypatch, fuse):
    cam = _camera()
    target = torch.rand(3, cam["height"], cam["width"], device=dev(), generator=torch.Generator(device=dev()).manual_seed(1))
    runs = []
    for use_oracle in (False, True):
        model = _scene_model()
        init = {k: v.detach().clone() for k, v in model.gaussians.items()}
        opts = model.make_optimizers(1.0, optimizers.FusedAdam, fuse_into_backward=fuse)
        loss = _render_step(model, opts, cam, target)
        loss.backward()
        for o in opts:
            o.step()
            o.zero_grad(set_to_none=True)
        gen = torch.Generator(device=dev()).manual_seed(5)
        with torch.no_grad():                  # the same state in both runs (the step's atomics may differ in the last bits)
            for o in opts:
                for grp in o.param_groups:
                    p = grp["params"][0]
                    p.copy_(init[grp["name"]])
                    st = o.state[p]
                    st["exp_avg"].copy_(torch.rand(p.shape, device=dev(), generator=gen) + 0.1)
                    st["exp_avg_sq"].copy_(torch.rand(p.shape, device=dev(), generator=gen) + 0.1)
        ctl = plugin.HipMCMCDensityController(cap_max=7000, densify_from_iter=0, densification_interval=1).instantiate()
        ctl.setup("validate", _Module(model, opts))
        sampled = []
        orig = ctl._sample_alives
        monkeypatch.setattr(ctl, "_sample_alives", lambda *a, **k: sampled.append(orig(*a, **k)) or sampled[-1])
        if use_oracle:
            monkeypatch.setattr(plugin._ops, "compute_relocation", _oracle_relocation)
        torch.manual_seed(2024)
        n0 = model.n_gaussians
        ctl.after_backward({}, None, model, opts, 1, None)
        monkeypatch.undo()
        assert model.n_gaussians == min(7000, int(1.05 * n0))
        # the rows the surgery touched have cleared moments, in every parameter's optimizer; the others kept theirs
        st = {grp["name"]: (o.state[grp["params"][0]], grp["params"][0]) for o in opts for grp in o.param_groups}
        for name, (s, p) in st.items():
            assert p is model.gaussians[name] and s["exp_avg"].shape == p.shape
            touched = torch.zeros(p.shape[0], dtype=torch.bool, device=dev())
            for idx, _ in sampled:
                assert not s["exp_avg"][idx].any() and not s["exp_avg_sq"][idx].any(), name
                touched[idx] = True
            touched[n0:] = True
            assert not s["exp_avg"][n0:].any() and bool((s["exp_avg"][~touched] >= 0.1).all()), name
        runs.append(({k: v.detach().clone() for k, v in model.gaussians.items()}, [i for i, _ in sampled]))
        # ... and training goes on with the surgically replaced parameters
        loss = _render_step(model, opts, cam, target)
        loss.backward()
        for o in opts:
            o.step()
        assert all(torch.isfinite(v).all() for v in model.gaussians.values())
    (hip, hip_idx), (ref, ref_idx) = runs
    assert len(hip_idx) == len(ref_idx) == 2 and all(torch.equal(a, b) for a, b in zip(hip_idx, ref_idx))
    for k in hip:
        if k in ("opacities", "scales"):      # relocated rows: oracle-close (log of the values), copied rows bit-equal
            assert torch.allclose(hip[k], ref[k], rtol=1e-5, atol=1e-5), k
        else:
            assert torch.equal(hip[k], ref[k]), k


def test_mcmc_training_run_reaches_cap_max():
    cam = _camera(160, 112)
    means, scales, quats, opac, shs = synthetic.scene(3000, seed=8)
    model = _Model(*(t.to(dev()) for t in bench_loop.perturbed((means, scales, quats, opac, shs))), active_sh_degree=3)
    with torch.no_grad():
        st = ops.GaussianRasterizationSettings(112, 160, cam["tanfovx"], cam["tanfovy"], torch.zeros(3, device=dev()), 1.0,
                                               cam["world_to_camera"], cam["full_projection"], 3, cam["camera_center"])
        d = [t.to(dev()) for t in (means, scales, quats, opac, shs)]
        target, _ = ops.GaussianRasterizer(st)(d[0], torch.zeros_like(d[0]), d[3].reshape(-1, 1), shs=d[4], scales=d[1], rotations=d[2])
    opts = model.make_optimizers(1.0, optimizers.FusedAdam)
    module = _Module(model, opts)
    ctl = plugin.HipMCMCDensityController(cap_max=4000, densify_from_iter=20, densification_interval=20, noise_lr=5e5).instantiate()
    ctl.setup("fit", module)
    assert module.on_train_batch_end_hooks == [ctl._add_xyz_noise]

    class _Metric:
        opacity_reg_weight, scale_reg_weight = 0.01, 0.01
    losses, counts = [], []
    torch.manual_seed(0)
    for step in range(1, 301):
        loss = _render_step(model, opts, cam, target)
        metrics = plugin.hip_reg_loss(_Metric, model, ({"loss": loss}, {}))
        metrics[0]["loss"].backward()
        ctl.after_backward({}, None, model, opts, step, module)
        for o in opts:
            o.step()
            o.zero_grad(set_to_none=True)
        for hook in module.on_train_batch_end_hooks:
            hook({}, None, model, step, module)
        losses.append(loss.item())
        counts.append(model.n_gaussians)
    assert counts[-1] == 4000 and all(torch.isfinite(v).all() for v in model.gaussians.values())
    assert np.mean(losses[-20:]) < 0.9 * np.mean(losses[:20]), (losses[:5], losses[-5:])

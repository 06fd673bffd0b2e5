"""Cost of the 3DGS-MCMC route's per-step extras, the reference's torch lines against this package's HIP ops.  Variants alternate round
by round inside ONE process so that clock and thermal drift spread over both.

  (i)   the full MCMC training step at each workload (default S-1080p-1M and S-1080p-6M; the heterogeneous 16-camera set, one camera
        per step): GaussianRasterizer on the raw parameters (what HipVanillaRenderer calls), L1 + SSIM, the MCMC regulariser, backward,
        FusedAdam, then the noise on the means —
          torch  the regulariser and `_add_xyz_noise` as the reference writes them (internal/metrics/mcmc_metrics.py `reg_loss`,
                 internal/density_controllers/mcmc_density_controller.py:93-119 with compute_cov_3d): activated getters, abs, mean;
                 zeros + nine indexed writes + bmm + matmul, randn_like, the steep sigmoid, a third bmm
          hip    ops.mcmc_regularization on the raw parameters and ops.perturb_means_ (the gspl_amd.mcmc plugin's calls)
  (ii)  the noise step alone, and the regulariser's forward + backward alone, torch vs hip;
  (iii) one relocation + growth event of HipMCMCDensityController at the first workload (5 % dead Gaussians), its compute_relocation
        launch timed on its own.

Prints one JSON line.  `--noise-only K` runs K noise launches and nothing else (for `rocprofv3 --kernel-trace --stats`), and prints the
bytes the kernel must move: 56 B per Gaussian (means read + written, scales, rotations, opacity).
  python tools/mcmc_step_time.py [--workloads S-1080p-1M,S-1080p-6M] [--rounds 5] [--steps 20] [--warmup 5]"""
import json
import time

import torch

import _step_time as T

NOISE_LR, MEANS_LR, REG_W = 5e5, 1.6e-4, 0.01
BYTES_PER_GAUSSIAN = 56


def _torch_cov3d(scales, quats):
    """compute_cov_3d's launch structure (gaussian_projection.py:211-254): a zeroed scaling matrix with its diagonal written, the
    rotation matrix written entry by entry, two batched products."""
    n = scales.shape[0]
    S = torch.zeros((n, 3, 3), dtype=scales.dtype, device=scales.device)
    for i in range(3):
        S[:, i, i] = scales[:, i]
    r, x, y, z = quats[:, 0], quats[:, 1], quats[:, 2], quats[:, 3]
    R = torch.zeros((n, 3, 3), dtype=quats.dtype, device=quats.device)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    m = torch.bmm(R, S)
    return torch.matmul(m, m.transpose(1, 2))


@torch.no_grad()
def torch_noise(g):
    cov = _torch_cov3d(torch.exp(g["scales"]), torch.nn.functional.normalize(g["rotations"]))
    op = torch.sigmoid(g["opacities"])
    noise = torch.randn_like(g["means"]) * (1 / (1 + torch.exp(-100 * ((1 - op) - 0.995)))) * NOISE_LR * MEANS_LR
    noise = torch.bmm(cov, noise.unsqueeze(-1)).squeeze(-1)
    g["means"].add_(noise)


def hip_noise(g):
    from gspl_amd import ops
    ops.perturb_means_(g["means"], g["scales"], g["rotations"], g["opacities"], raw=True, noise_scale=NOISE_LR * MEANS_LR)


def torch_reg(g):
    return REG_W * torch.abs(torch.sigmoid(g["opacities"])).mean() + REG_W * torch.abs(torch.exp(g["scales"])).mean()


def hip_reg(g):
    from gspl_amd import ops
    o, s = ops.mcmc_regularization(g["opacities"], g["scales"], REG_W, REG_W, raw=True)
    return o + s


def main():
    p = T.arguments(steps=20, warmup=5)
    p.add_argument("--workloads", default="S-1080p-1M,S-1080p-6M")
    p.add_argument("--noise-only", type=int, default=0)
    a = p.parse_args()
    import gspl_amd  # noqa: F401
    import bench_loop
    from gspl_amd import ops, optimizers, synthetic
    from gspl_amd import mcmc as plugin
    assert torch.cuda.is_available(), "mcmc_step_time measures on the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    result = {"tool": "mcmc_step_time", "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup, "bytes_per_gaussian_noise": BYTES_PER_GAUSSIAN}

    def model_for(wl):
        return bench_loop.RawGaussians(*T.scene(wl, dev), active_sh_degree=3)

    workloads = [w for w in a.workloads.split(",") if w]
    if a.noise_only:
        wl = synthetic.WORKLOADS[workloads[0]]
        g = model_for(wl).gaussians
        with torch.no_grad():
            for _ in range(a.noise_only):
                hip_noise(g)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "mcmc_step_time", "noise_only": a.noise_only, "workload": workloads[0], "n": wl["n"],
                          "bytes_per_launch": BYTES_PER_GAUSSIAN * wl["n"]}))
        return

    for wname in workloads:
        w = T.load(wname, dev)
        wl, W, H, cams, order, bg, target = w.wl, w.W, w.H, w.cams, w.order, w.bg, w.target
        models = {v: model_for(wl) for v in ("torch", "hip")}
        opts = {v: models[v].make_optimizers(1.0, optimizers.FusedAdam) for v in models}
        reg = {"torch": torch_reg, "hip": hip_reg}
        noise = {"torch": torch_noise, "hip": hip_noise}
        k = [0]

        def step(v):
            g = models[v].gaussians
            cam = cams[order[k[0] % len(order)]]
            k[0] += 1
            st = ops.GaussianRasterizationSettings(H, W, cam["tanfovx"], cam["tanfovy"], bg, 1.0, cam["world_to_camera"], cam["full_projection"], 3,
                                                   cam["camera_center"])
            screen = torch.empty_like(g["means"]).requires_grad_(True)
            img, _ = ops.GaussianRasterizer(st)(g["means"], screen, g["opacities"], shs=g["shs_dc"], shs_rest=g["shs_rest"], scales=g["scales"],
                                                rotations=g["rotations"], raw_parameters=True)
            l1, ssim = ops.l1_ssim(img, target)
            loss = 0.8 * l1 + 0.2 * (1 - ssim) + reg[v](g)
            loss.backward()
            for o in opts[v]:
                o.step()
                o.zero_grad(set_to_none=True)
            noise[v](g)

        def noise_alone(v):
            noise[v](models[v].gaussians)

        def reg_alone(v):
            g = models[v].gaussians
            reg[v](g).backward()
            for t in g.values():
                t.grad = None

        rec = {}
        for name, fn in (("step", step), ("noise", noise_alone), ("regulariser", reg_alone)):
            med, med_print, rounds_print = T.medians(T.alternate(("torch", "hip"), lambda v, _i: fn(v), a.rounds, a.steps, a.warmup))
            rec[name] = {"ms_median": med_print, "ms_rounds": rounds_print, "saving_ms": round(med["torch"] - med["hip"], 4)}
        rec["noise"]["hip_achieved_GBps_from_event_time"] = round(BYTES_PER_GAUSSIAN * wl["n"] / (rec["noise"]["ms_median"]["hip"] * 1e-3) / 1e9, 1)
        result[wname] = {"n": wl["n"], **rec}
        del models, opts
        torch.cuda.empty_cache()

    # (iii) one relocation + growth event at the first workload
    wl = synthetic.WORKLOADS[workloads[0]]
    model = model_for(wl)

    class _Model(type(model)):
        properties = property(lambda s: s.gaussians, lambda s, v: setattr(s, "gaussians", dict(v)))
        opacity_inverse_activation = staticmethod(lambda o: torch.log(o / (1 - o)))
        scale_inverse_activation = staticmethod(torch.log)
    model.__class__ = _Model
    opts = model.make_optimizers(1.0, optimizers.FusedAdam)
    for o in opts:
        for grp in o.param_groups:
            pp = grp["params"][0]
            o.state[pp] = {"step": 1, "exp_avg": torch.zeros_like(pp), "exp_avg_sq": torch.zeros_like(pp)}
    with torch.no_grad():
        dead = torch.rand(model.n_gaussians, device=dev) < 0.05
        model.gaussians["opacities"][dead] = -8.0

    class _Module:
        device, gaussian_model, gaussian_optimizers, on_train_batch_end_hooks = dev, model, opts, []
    ctl = plugin.HipMCMCDensityController(cap_max=10 * wl["n"], densify_from_iter=0, densification_interval=1).instantiate()
    ctl.setup("validate", _Module)
    reloc_ms = []
    orig = ctl.compute_relocation

    def timed_relocation(*args, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig(*args, **kw)
        e1.record()
        reloc_ms.append((e0, e1))
        return out
    ctl.compute_relocation = timed_relocation
    n0 = model.n_gaussians
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctl.after_backward({}, None, model, opts, 1, _Module)
    torch.cuda.synchronize()
    event_ms = (time.perf_counter() - t0) * 1e3
    result["relocation_event"] = {"workload": workloads[0], "n_before": n0, "n_after": model.n_gaussians, "dead": int(dead.sum()),
                                  "event_ms_host_clock": round(event_ms, 3),
                                  "compute_relocation_ms": [round(e0.elapsed_time(e1), 4) for e0, e1 in reloc_ms]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()

"""Worker of tests/test_mcmc_loop.py (its own process: the `lightning` stand-in must not leak into the other tests' imports of the
reference tree).

Runs the reference's UNCHANGED LightningModule (`internal/gaussian_splatting.py`: `setup("fit")`, `configure_optimizers`,
`on_train_start`, then `on_train_batch_start` / `training_step` / `on_train_batch_end` per batch) with its own `Cameras`,
`VanillaGaussian` model, optimizers and schedulers, and with the 3DGS-MCMC route selected the way
`--model.density gspl_amd.mcmc.HipMCMCDensityController --model.metric gspl_amd.mcmc.HipMCMCMetrics
--model.renderer gspl_amd.renderers.HipVanillaRenderer` does it (the constructor arguments `density=`, `metric=`, `renderer=`).

No GPU here: the plugins' native ops run on the fp64 oracles — `ops.GaussianRasterizer` on `oracle.render_inria`, the three MCMC ops of
`gspl_amd.ops.mcmc` on tests/mcmc_oracle.py (normals from torch's CPU generator) — and every call is counted.  Everything else is the
code a training run executes.  Prints one JSON line: per step the loss, the Gaussian count, the noise and regulariser calls, and per
relocation event what the controller did.
usage: python mcmc_loop_worker.py <reference root> <steps> [raw | activated]
  raw        the reference's vanilla model as it is: its raw parameters go to the kernels (renderers.renderer.model_raw_parameters)
  activated  the same run with that recognition switched off: the plugins read `get_scales()` / `get_opacity` ... as for any other model
"""
import json
import math
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_ROOT, STEPS = sys.argv[1], int(sys.argv[2])
VARIANT = sys.argv[3] if len(sys.argv) > 3 else "raw"
for p in (REF_ROOT, HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lightning_standin  # noqa: E402

lightning_standin.install()

import gspl_amd  # noqa: E402,F401
from gspl_amd import compat, ops  # noqa: E402
from gspl_amd import mcmc as plugin  # noqa: E402
from gspl_amd.renderers import HipVanillaRenderer  # noqa: E402
from oracle import gsplat_oracle as O  # noqa: E402
from oracle import knn_oracle  # noqa: E402
import mcmc_oracle as MO  # noqa: E402

compat.install()

from internal.gaussian_splatting import GaussianSplatting  # noqa: E402  (the reference's LightningModule, unchanged)
from internal.cameras.cameras import Cameras  # noqa: E402
from internal.configs.light_gaussian import LightGaussian  # noqa: E402
from internal.density_controllers.density_controller import DensityControllerImpl as ReferenceDensityControllerImpl  # noqa: E402
from internal.metrics.mcmc_metrics import MCMCMetricsImpl  # noqa: E402
from internal.models.vanilla_gaussian import VanillaGaussian  # noqa: E402
from internal.optimizers import Adam  # noqa: E402
from internal.schedulers import ExponentialDecayScheduler  # noqa: E402

W_IMG, H_IMG, FOCAL = 160, 112, 150.0
EXTENT = 4.4
CALLS = {"noise": 0, "noise_raw": 0, "reg": 0, "reg_raw": 0, "relocation": 0}


class OracleRasterizer:
    """Stands in for `ops.GaussianRasterizer` (the fused Inria call): same arguments and returns, `.grad` of the screen-space carrier in
    the Inria (NDC-scaled) units."""

    def __init__(self, raster_settings):
        self.s = raster_settings

    def __call__(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None,
                 shs_rest=None, raw_parameters=False):
        s = self.s
        if raw_parameters:
            opacities, scales, rotations = torch.sigmoid(opacities), torch.exp(scales), torch.nn.functional.normalize(rotations)
        if shs_rest is not None:
            shs = torch.cat((shs, shs_rest), dim=1)
        r = O.render_inria(means3D, scales, rotations, opacities, shs, s.sh_degree, s.viewmatrix, s.projmatrix, s.campos,
                           s.tanfovx, s.tanfovy, s.image_width, s.image_height, s.bg)
        sc = torch.tensor([0.5 * s.image_width, 0.5 * s.image_height])
        if r["xy"].requires_grad:
            r["xy"].register_hook(lambda g: setattr(means2D, "grad", torch.cat([g * sc, torch.zeros_like(g[:, :1])], dim=1)))
        return r["render"], r["radii"]


# ---- the MCMC ops on the oracle ------------------------------------------------------------------------------------------------------
def oracle_relocation(opacities, scales, ratios, binoms):
    CALLS["relocation"] += 1
    o, s, _ = MO.relocation(opacities.double().numpy(), scales.double().numpy(), ratios.numpy(), binoms.shape[0])
    return torch.tensor(o, dtype=torch.float32), torch.tensor(s, dtype=torch.float32)


@torch.no_grad()
def oracle_perturb_means_(means, scales, rotations, opacities, *, raw, noise_scale, noise=None, generator=None):
    CALLS["noise"] += 1
    CALLS["noise_raw"] += int(bool(raw))
    eps = torch.randn(means.shape, dtype=torch.float64) if noise is None else noise.double()
    new = MO.perturb(means.numpy(), scales.numpy(), rotations.numpy(), opacities.numpy(), eps.numpy(), noise_scale, raw)
    means.copy_(torch.from_numpy(new))
    return means


class _OracleReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opacities, scales, opacity_w, scale_w, raw):
        ctx.save_for_backward(opacities, scales)
        ctx.cfg = (opacity_w, scale_w, raw)
        o, s = MO.reg_fwd(opacities.detach().numpy(), scales.detach().numpy(), opacity_w, scale_w, raw)
        return torch.tensor([o, s], dtype=torch.float32)

    @staticmethod
    def backward(ctx, g):
        opacities, scales = ctx.saved_tensors
        vo, vs = MO.reg_bwd(opacities.detach().numpy(), scales.detach().numpy(), *ctx.cfg, float(g[0]), float(g[1]))
        return torch.from_numpy(vo).float(), torch.from_numpy(vs).float(), None, None, None


def oracle_regularization(opacities, scales, opacity_w, scale_w, *, raw):
    CALLS["reg"] += 1
    CALLS["reg_raw"] += int(bool(raw))
    out = _OracleReg.apply(opacities, scales, opacity_w, scale_w, raw)
    return out[0], out[1]


def orbit_cameras(n=6):
    """The reference's own `Cameras` container: n views on a circle of radius 4 about the y axis, looking at the origin."""
    Rs, Ts = [], []
    for i in range(n):
        a = 2 * math.pi * i / n
        c, s = math.cos(a), math.sin(a)
        Rs.append(torch.tensor([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]]))
        Ts.append(torch.tensor([0.0, 0.0, 4.0]))
    f = lambda v, dt=torch.float32: torch.full((n,), v, dtype=dt)
    return Cameras(R=torch.stack(Rs), T=torch.stack(Ts), fx=f(FOCAL), fy=f(FOCAL), cx=f(W_IMG / 2), cy=f(H_IMG / 2),
                   width=f(W_IMG, torch.int32), height=f(H_IMG, torch.int32), appearance_id=f(0, torch.int32),
                   normalized_appearance_id=f(0.0), distortion_params=None, camera_type=f(0, torch.int32))


def main():
    assert plugin.INSIDE_REFERENCE, "the controller must subclass the reference's own DensityControllerImpl here"
    plugin._ops.compute_relocation = oracle_relocation
    plugin._ops.perturb_means_ = oracle_perturb_means_
    plugin._ops.mcmc_regularization = oracle_regularization
    if VARIANT == "activated":
        plugin.model_raw_parameters = lambda pc: None

    g = torch.Generator().manual_seed(9)
    n_gt = 600
    gt = dict(means=(torch.rand(n_gt, 3, generator=g) * 2 - 1) * 0.9, scales=torch.exp(torch.randn(n_gt, 3, generator=g) * 0.3 - 2.3),
              quats=torch.nn.functional.normalize(torch.randn(n_gt, 4, generator=g), dim=-1), opac=torch.rand(n_gt, 1, generator=g) * 0.5 + 0.45,
              shs=torch.cat([torch.randn(n_gt, 1, 3, generator=g) * 0.8, torch.randn(n_gt, 15, 3, generator=g) * 0.05], dim=1))
    cameras = orbit_cameras()
    bg = torch.zeros(3)
    targets = []
    with torch.no_grad():
        for cam in cameras:
            r = O.render_inria(gt["means"], gt["scales"], gt["quats"], gt["opac"], gt["shs"], 3, cam.world_to_camera, cam.full_projection,
                               cam.camera_center, math.tan(float(cam.fov_x) / 2), math.tan(float(cam.fov_y) / 2), W_IMG, H_IMG, bg)
            targets.append(r["render"].float().clamp(0, 1))
    n0 = 1500
    pick = torch.randint(0, n_gt, (n0,), generator=g)
    xyz = (gt["means"][pick] + 0.05 * torch.randn(n0, 3, generator=g)).numpy()
    rgb = ((gt["shs"][pick, 0] * 0.28209479177387814 + 0.5).clamp(0, 1) * 255).numpy()

    ops.GaussianRasterizer = OracleRasterizer
    sys.modules["simple_knn._C"].distCUDA2 = lambda pts: torch.from_numpy(knn_oracle.mean_dist2_kdtree(pts.detach().cpu().numpy().astype(np.float64))).float()
    torch.Tensor.cuda = lambda self, *a, **k: self            # `setup_from_pcd` moves the points to "cuda" for distCUDA2 (vanilla_gaussian.py:124)

    cap_max = 2000
    density = plugin.HipMCMCDensityController(cap_max=cap_max, densify_from_iter=25, densification_interval=25, densify_until_iter=280,
                                              min_opacity=0.1)
    metric = plugin.HipMCMCMetrics(opacity_reg=0.01, scale_reg=0.01)
    gaussian = VanillaGaussian(sh_degree=3)
    gaussian.optimization.sh_degree_up_interval = 60
    gaussian.optimization.optimizer = Adam()
    gaussian.optimization.means_lr_scheduler = ExponentialDecayScheduler(lr_final=0.0000016, max_steps=STEPS)
    module = GaussianSplatting(light_gaussian=LightGaussian(), save_iterations=[], gaussian=gaussian, renderer=HipVanillaRenderer(),
                               metric=metric, density=density, output_path=tempfile.mkdtemp(prefix="gspl_mcmc_loop_"))

    ns = lambda **kw: type("NS", (), kw)()
    datamodule = ns(point_cloud=ns(xyz=xyz, rgb=rgb), prune_extent=EXTENT,
                    dataparser_outputs=ns(camera_extent=EXTENT, train_set=ns(cameras=cameras, image_names=[f"{i:03d}" for i in range(len(cameras))]),
                                          val_set=ns(cameras=cameras)),
                    set_device=lambda device: None)
    trainer = lightning_standin.Trainer(datamodule, max_steps=STEPS)
    loader = ns(dataset=ns(image_cameras=list(cameras)))
    trainer.train_dataloader, trainer.val_dataloaders = loader, loader
    trainer.fit_setup(module)
    ctl, mtr, model = module.density_controller, module.metric, module.gaussian_model
    assert isinstance(ctl, plugin.HipMCMCDensityControllerImpl) and isinstance(ctl, ReferenceDensityControllerImpl)
    assert isinstance(mtr, plugin.HipMCMCMetricsImpl) and isinstance(mtr, MCMCMetricsImpl)
    hooks = [h for h in module.on_train_batch_end_hooks if getattr(h, "__func__", None) is plugin.HipMCMCDensityControllerImpl._add_xyz_noise]
    init_opacity = float(model.get_opacities().mean())             # setup("fit"): every opacity 0.5

    # record what every event does, around the controller's own methods
    events, sampled = [], []
    relocate, add_new, sample = ctl.relocate_gs, ctl.add_new_gs, ctl._sample_alives
    def _sample(a, k):
        out = sample(*a, **k)
        sampled.append(out[0])
        return out
    ctl._sample_alives = lambda *a, **k: _sample(a, k)

    def relocate_gs(gaussian_model, optimizers, dead_mask):
        sampled.clear()
        means0 = gaussian_model.get_property("means").detach().clone()
        dead = dead_mask.nonzero(as_tuple=True)[0]
        relocate(gaussian_model, optimizers, dead_mask)
        ev = {"n_before": int(gaussian_model.n_gaussians), "dead": int(dead.numel()), "dead_rows_replaced": True, "touched": dead.tolist()}
        if dead.numel() > 0:
            src = sampled[0]
            ev["dead_rows_replaced"] = bool(torch.equal(gaussian_model.get_property("means")[dead], means0[src]))
            ev["touched"] += src.tolist()
        events.append(ev)

    def add_new_gs(gaussian_model, optimizers):
        n_before = gaussian_model.n_gaussians
        sampled.clear()
        added = add_new(gaussian_model, optimizers)
        ev = events[-1]
        ev["n_after"] = int(gaussian_model.n_gaussians)
        ev["added"] = int(added)
        touched = torch.zeros(ev["n_after"], dtype=torch.bool)
        touched[torch.tensor(ev.pop("touched"), dtype=torch.long)] = True
        if sampled:
            touched[sampled[0]] = True
        touched[n_before:] = True
        low = (gaussian_model.get_opacities().squeeze(-1) <= ctl.config.min_opacity)
        ev["low_opacity_untouched"] = int((low & ~touched).sum())
        return added
    ctl.relocate_gs, ctl.add_new_gs = relocate_gs, add_new_gs

    losses, counts, noise_calls, reg_calls, o_regs = [], [], [], [], []
    for i in range(STEPS):
        torch.manual_seed(1000 + i)
        k = i % len(cameras)
        batch = (cameras[k], (f"{k:03d}", targets[k], None), None)
        trainer.train_batch(module, batch, i)
        assert trainer.global_step == i + 1
        losses.append(module.logged["train/loss"])
        o_regs.append(float(module.logged.get("train/o_reg", float("nan"))))
        counts.append(int(module.gaussian_model.get_xyz.shape[0]))
        noise_calls.append(CALLS["noise"])
        reg_calls.append(CALLS["reg"])
    means_lr = float(trainer.raw_optimizers[0].param_groups[0]["lr"])
    print(json.dumps({"variant": VARIANT, "losses": losses, "counts": counts, "noise_calls": noise_calls, "reg_calls": reg_calls, "o_regs": o_regs,
                      "calls": CALLS, "events": events, "cap_max": cap_max, "n0": n0, "steps": STEPS, "hooks": len(hooks),
                      "init_opacity": init_opacity, "densify": {"from": 25, "interval": 25, "until": 280}, "means_lr_last": means_lr,
                      "metric": type(mtr).__module__ + "." + type(mtr).__name__,
                      "controller": type(ctl).__module__ + "." + type(ctl).__name__}))


if __name__ == "__main__":
    main()

"""Forward + backward of a Periodic-Vibration-Gaussian frame: `HipPeriodicVibrationGaussianRenderer` against the reference renderer's
call sequence restated on the ops that existed before it.  One process, the two routes alternating repeat by repeat so that clock and
thermal drift spread over both.

  plugin    one `ops.pvg_motion`, one projection, one binning, one D = 8 compositing pass, `ops.envlight_blend`
  restated  the motion, the opacity factor and the average velocity in elementwise torch (the model's getters); one
            `ops.rasterize_gaussians` call per map (rgb with alpha, average velocity), each with its own binning and geometry backward;
            with the sky on: a full-frame direction grid in torch, the cube map sampled by a torch gather restatement of the sampler
            (tests/pvg_oracle.py, float32) and the three-operand blend in torch

Workload: S-800-100k (100 000 Gaussians at 800x800) with seeded PVG rows (velocity, life peak, lifespan), the default render types
(rgb and average_velocity), the loss 0.8 L1 + 0.001 mean |average_velocity / alpha| of pvg_dynamic_metrics.  `env_map_res` 0 (no sky)
and 1024.  Per repeat the MEDIAN of `--steps` steps, each timed with its own pair of device events; `--repeats` repeats per route.
The plugin is called faster when its slowest repeat beats the restated route's fastest.  Prints one JSON line.
  python tools/pvg_step_time.py [--env-map-res 0,1024] [--steps 20] [--warmup 5] [--repeats 3]"""
import argparse
import json
import math
import os
import statistics
import sys
import types

import _step_time as T  # noqa: F401  (puts the repository root on sys.path)
import torch

sys.path.insert(0, os.path.join(T.ROOT, "tests"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--workload", default="S-800-100k")
    p.add_argument("--env-map-res", default="0,1024")
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=3)
    a = p.parse_args()
    import gspl_amd  # noqa: F401
    from gspl_amd import ops, synthetic
    from gspl_amd.renderers import HipGSplatRenderer, HipPeriodicVibrationGaussianRenderer
    import pvg_oracle as PO
    assert torch.cuda.is_available(), "pvg_step_time measures on the GPU"
    assert a.steps >= 1 and a.repeats >= 1
    dev = torch.device("cuda:0")
    wl = synthetic.WORKLOADS[a.workload]
    W, H, n = wl["width"], wl["height"], wl["n"]
    means, scales, quats, opac, shs = T.scene(wl, dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    cycle, decay, offset = 0.2, 1.0, -0.5
    P = lambda t: t.clone().requires_grad_(True)
    model = types.SimpleNamespace(
        means=P(means), velocity=P(torch.randn(n, 3, device=dev, generator=gen) * 0.3),
        t=P(torch.rand(n, 1, device=dev, generator=gen) * 1.2 - 0.6), scale_t=P(torch.exp(-2.0 * torch.rand(n, 1, device=dev, generator=gen))),
        opacities=P(opac), scales=scales, quats=quats, shs=shs, active_sh_degree=3, is_pre_activated=False,
        config=types.SimpleNamespace(cycle=cycle, velocity_decay=decay, time_duration=(-0.5, 0.5)))
    model.get_means, model.get_velocity, model.get_t = (lambda: model.means), (lambda: model.velocity), (lambda: model.t)
    model.get_scale_t, model.get_opacities = (lambda: model.scale_t), (lambda: model.opacities)
    model.get_xyz, model.get_scaling, model.get_rotation, model.get_features = model.means, scales, quats, shs
    leaves = [model.means, model.velocity, model.t, model.scale_t, model.opacities]
    cam = synthetic.camera(W, H, wl["fx"])

    class Camera:
        world_to_camera = cam["world_to_camera"].to(dev)
        camera_center = cam["camera_center"].to(dev)
        fx, fy, cx, cy = (torch.tensor(float(cam[k]), device=dev) for k in ("fx", "fy", "cx", "cy"))
        width, height = torch.tensor(W, device=dev), torch.tensor(H, device=dev)
        time = torch.tensor(0.62, device=dev)
    camera = Camera()
    bg = torch.zeros(3, device=dev)
    target = torch.rand(3, H, W, device=dev, generator=gen)
    c2w = torch.linalg.inv(camera.world_to_camera.T)[:3, :3].contiguous()
    result = {"tool": "pvg_step_time", "workload": a.workload, "n": n, "width": W, "height": H, "steps": a.steps, "warmup": a.warmup,
              "repeats": a.repeats, "render_types": ["rgb", "average_velocity"]}

    def loss_of(out):
        v_reg = (out["average_velocity"] / out["alpha"].detach().clamp_min(1e-5)).abs().mean() * 0.001
        return 0.8 * (out["render"] - target).abs().mean() + v_reg

    for res in [int(r) for r in a.env_map_res.split(",") if r != ""]:
        renderer = HipPeriodicVibrationGaussianRenderer(env_map_res=res).instantiate()
        renderer.setup("fit")
        renderer.to(dev).eval()          # pixel centres on both routes: the jitter is the same torch.rand either way
        base = None
        if res > 0:
            with torch.no_grad():
                renderer.env_map.base.copy_(torch.rand(6, res, res, 3, device=dev, generator=gen))
            base = renderer.env_map.base
            leaves_now = leaves + [base]
        else:
            leaves_now = leaves

        def plugin():
            return renderer(camera, model, bg)

        def restated():
            ts = camera.time + offset
            k = 1 / cycle * math.pi * 2
            means3D = model.means + model.velocity * torch.sin((ts - model.t) * k) / k
            marginal = torch.exp(-0.5 * (model.t - ts) ** 2 / model.scale_t ** 2)
            average_velocity = model.velocity * torch.exp(-model.scale_t / cycle / 2 * decay)
            opacities = model.opacities * marginal
            proj = HipGSplatRenderer.project(means3D, scales, quats, camera)
            xys, depths, radii, conics, comp, tiles, _ = proj
            opacities = opacities * comp[:, None]
            rgbs = ops.sh_view_colors(3, model.means, camera.camera_center, shs, None, radii > 0, detach_means=True)
            raster = lambda colors, background, **kw: ops.rasterize_gaussians(xys, depths, radii, conics, tiles, colors, opacities, H, W, 16,
                                                                              background=background, **kw)
            rgb, alpha = raster(rgbs, bg, return_alpha=True)
            alpha = alpha.unsqueeze(-1)
            if base is not None:
                v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                                      indexing="ij")
                d = torch.stack([(u - camera.cx + 0.5) / camera.fx, (v - camera.cy + 0.5) / camera.fy, torch.ones_like(u)], dim=0)
                d = torch.nn.functional.normalize(d, dim=0)
                d = (c2w @ d.reshape(3, -1)).reshape(3, H, W).permute(1, 2, 0)
                l = torch.stack([d[..., 0], d[..., 2], -d[..., 1]], dim=-1)
                rgb = rgb + (1 - alpha) * PO.cubemap(base, l.reshape(-1, 3)).reshape(H, W, 3)
            velocity_map = raster(average_velocity, torch.zeros(3, device=dev))
            return {"render": rgb.permute(2, 0, 1), "alpha": alpha.permute(2, 0, 1), "average_velocity": velocity_map.permute(2, 0, 1)}

        routes = {"restated": restated, "plugin": plugin}

        def step(fn):
            for leaf in leaves_now:
                leaf.grad = None
            loss_of(fn()).backward()

        # the two routes compute the same frame and the same gradients, to rounding, at the size that is timed
        step(restated)
        grads_restated = [leaf.grad.clone() for leaf in leaves_now]
        with torch.no_grad():
            frame_diff = float((restated()["render"] - plugin()["render"]).abs().max())
        step(plugin)
        grad_diff = max(float(((leaf.grad - g).abs() / (g.abs() + g.square().mean().sqrt() + 1e-30)).max()) for leaf, g in zip(leaves_now, grads_restated))
        del grads_restated

        medians = {name: [] for name in routes}
        for r in range(a.repeats):
            for name in (list(routes) if r % 2 == 0 else list(routes)[::-1]):
                for _ in range(a.warmup):
                    step(routes[name])
                torch.cuda.synchronize()
                events = []
                for _ in range(a.steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    step(routes[name])
                    e1.record()
                    events.append((e0, e1))
                torch.cuda.synchronize()
                medians[name].append(statistics.median(e0.elapsed_time(e1) for e0, e1 in events))
        result[f"env_map_res_{res}"] = {
            "ms_per_step_median_of_repeats": {k: round(statistics.median(v), 4) for k, v in medians.items()},
            "ms_per_step_repeats": {k: [round(x, 4) for x in v] for k, v in medians.items()},
            "spread_of_repeats_ms": {k: round(max(v) - min(v), 4) for k, v in medians.items()},
            "speedup": round(statistics.median(medians["restated"]) / statistics.median(medians["plugin"]), 3),
            "plugin_faster_beyond_spread": max(medians["plugin"]) < min(medians["restated"]),
            "worst_frame_difference": frame_diff, "worst_gradient_difference_rel": grad_diff,
        }
        del renderer
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()

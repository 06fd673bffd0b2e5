"""The 3D half of the Mip-Splatting route: `ops.mip_filter_3d` and `ops.mip_apply_3d_filter` (csrc/mip.hip) against the reference's
formulation, `MipSplattingUtils.compute_3d_filter` / `apply_3d_filter` restated below operation by operation in float32 torch ops, on
the same GPU, in one process, the two routes alternating repeat by repeat.  The parent commit has no such route: these comparisons are
against the reference's formulation, not against earlier code of this package.

(a) One filter event at N = 100 000 and 1 000 000 with C = 100 and 300 cameras on a ring around the cloud (cameras on the device, as
    the reference's `training_setup` leaves them): WALL time of the whole call, the device idle before and after, because the torch
    loop's cost is host waits as much as launches.  `host_waits`: the synchronising calls of one event, counted with
    `torch.cuda.set_sync_debug_mode("warn")`.
(b) `apply` forward + backward (gradients into raw scales and raw opacities) at the same N, against the torch expression on the
    activated getters (exp and sigmoid in front), device time by events; a sample runs the route as often as it takes to fill ~20 ms.
(c) The plugin: `HipGSplatMipSplattingRendererV2` on S-800-100k (100 000 Gaussians, 800 x 800), forward + backward of an L1 loss,
    against the same plugin with the torch expression in the mixin.
`worst_difference`: the two routes' results.  These are whole calls, host work included; the kernels alone are not measured here.

Each run of this command APPENDS to `runs` in the output file; `verdict` is computed over every run in it: a route counts as faster
only where its slowest repeat of any run is below the other's fastest.  The process ends itself after `--time-limit` seconds.
  python tools/mip_time.py [--steps 5] [--warmup 2] [--repeats 3] [--out profiles/mip_time.json]"""
import argparse
import json
import math
import os
import signal
import statistics
import time
import types
import warnings

import _step_time as T  # noqa: F401  (puts the repository root on sys.path)
import torch

SIZES = (100_000, 1_000_000)
CAMERAS = (100, 300)
WORKLOAD = "S-800-100k"


def torch_compute_3d_filter(cameras, xyz):
    """`MipSplattingUtils.compute_3d_filter`, operation by operation."""
    distance = torch.ones((xyz.shape[0]), device=xyz.device) * 100000.0
    valid_points = torch.zeros((xyz.shape[0]), device=xyz.device, dtype=torch.bool)
    focal_length = 0.
    for camera in cameras:
        R = camera.R.T.to(xyz.device)
        T_ = camera.T.to(xyz.device)
        xyz_cam = xyz @ R + T_[None, :]
        valid_depth = xyz_cam[:, 2] > 0.01
        x, y, z = xyz_cam[:, 0], xyz_cam[:, 1], xyz_cam[:, 2]
        z = torch.clamp(z, min=0.001)
        x = x / z * camera.fx + camera.width / 2.0
        y = y / z * camera.fy + camera.height / 2.0
        in_screen = torch.logical_and(torch.logical_and(x >= -0.15 * camera.width, x <= camera.width * 1.15),
                                      torch.logical_and(y >= -0.15 * camera.height, y <= 1.15 * camera.height))
        valid = torch.logical_and(valid_depth, in_screen)
        distance[valid] = torch.min(distance[valid], z[valid])
        valid_points = torch.logical_or(valid_points, valid)
        if focal_length < camera.fx:
            focal_length = camera.fx
    distance[~valid_points] = distance[valid_points].max()
    filter_3d = distance / focal_length * (0.2 ** 0.5)
    return filter_3d[..., None]


def torch_apply_3d_filter(filter_3d, opacities, scales, opacity_compensation=True):
    """`MipSplattingUtils.apply_3d_filter`, operation by operation."""
    scales_square = torch.square(scales)
    scales_after_square = scales_square + torch.square(filter_3d)
    new_opacities = opacities
    if opacity_compensation:
        det1 = scales_square.prod(dim=1)
        det2 = scales_after_square.prod(dim=1)
        coef = torch.sqrt(det1 / det2)
        new_opacities = opacities * coef[..., None]
    return new_opacities, torch.sqrt(scales_after_square)


def ring_cameras(C, dev):
    """C cameras on a ring of radius 3 around the unit cloud, looking at the origin, every field a tensor on the device."""
    out = []
    for i in range(C):
        a = 2 * math.pi * i / C
        position = torch.tensor([3 * math.cos(a), 0.3 * math.sin(3 * a), 3 * math.sin(a)], dtype=torch.float64)
        forward = -position / position.norm()
        right = torch.linalg.cross(forward, torch.tensor([0.0, -1.0, 0.0], dtype=torch.float64))
        right = right / right.norm()
        R = torch.stack([right, torch.linalg.cross(forward, right), forward])
        t = lambda v, dt=torch.float32: torch.as_tensor(v).to(device=dev, dtype=dt)
        out.append(types.SimpleNamespace(R=t(R), T=t(-R @ position), fx=t(600.0 + i), fy=t(600.0 + i), width=t(800, torch.int32), height=t(600, torch.int32)))
    return out


def _sample_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def _median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    inner = max(1, min(200, math.ceil(20.0 / max(_sample_ms(fn, 1), 1e-3))))
    return statistics.median(_sample_ms(fn, inner) for _ in range(steps))


def _wall_ms(fn, steps, warmup):
    samples = []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(samples[warmup:])


def _alternate(routes, steps, warmup, repeats, timer=_median_ms):
    times = {k: [] for k in routes}
    for rep in range(repeats):
        for k in (list(routes) if rep % 2 == 0 else list(routes)[::-1]):
            times[k].append(timer(routes[k], steps, warmup))
    return times


def _summary(times):
    return {"ms_median_of_repeats": {k: round(statistics.median(v), 4) for k, v in times.items()},
            "ms_repeats": {k: [round(t, 4) for t in v] for k, v in times.items()}}


def _host_waits(fn):
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(previous)
    return sum("synchroniz" in str(w.message).lower() for w in caught)


def measure_filter(n, C, a, dev):
    from gspl_amd import ops
    gen = torch.Generator().manual_seed(17)
    means = (torch.rand(n, 3, generator=gen) * 2 - 1).to(dev)
    means[: n // 50, 1] += 200.0                                  # 2 % that no camera sees
    cameras = ring_cameras(C, dev)
    table = ops.mip_camera_table(cameras, dev)
    routes = {"torch": lambda: torch_compute_3d_filter(cameras, means), "hip": lambda: ops.mip_filter_3d(means, table)}
    values = {k: fn() for k, fn in routes.items()}
    waits = {k: _host_waits(fn) for k, fn in routes.items()}
    times = _alternate(routes, min(a.steps, 3), 1, a.repeats, timer=_wall_ms)
    relative = ((values["hip"] - values["torch"]).abs() / values["torch"]).max()
    return {"N": n, "cameras": C, "wall": _summary(times), "host_waits": waits, "rows_differing": int((values["hip"] != values["torch"]).sum()),
            "worst_relative_difference": float(relative)}


def measure_apply(n, a, dev):
    from gspl_amd import ops
    gen = torch.Generator().manual_seed(11)
    raw_s = (torch.randn(n, 3, generator=gen) - 4).to(dev).requires_grad_(True)
    raw_o = (2 * torch.randn(n, 1, generator=gen)).to(dev).requires_grad_(True)
    f = (0.001 + 0.05 * torch.rand(n, 1, generator=gen)).to(dev)
    vs, vo = torch.randn(n, 3, generator=gen).to(dev), torch.randn(n, 1, generator=gen).to(dev)

    def hip():
        scales, opacities = ops.mip_apply_3d_filter(raw_s, f, raw_o, raw_scales=True, raw_opacities=True)
        return opacities, scales
    routes = {"torch": lambda: torch_apply_3d_filter(f, torch.sigmoid(raw_o), torch.exp(raw_s)), "hip": hip}

    def forward(route):
        def run():
            with torch.no_grad():
                return routes[route]()
        return run

    def step(route):
        def run():
            raw_s.grad = raw_o.grad = None
            opacities, scales = routes[route]()
            ((scales * vs).sum() + (opacities * vo).sum()).backward()
        return run
    values, grads = {}, {}
    for k in routes:
        step(k)()
        values[k], grads[k] = forward(k)(), (raw_s.grad.clone(), raw_o.grad.clone())
    difference = max(float((h - t).abs().max()) for h, t in zip(values["hip"], values["torch"]))
    gradient_difference = max(float((g - t).abs().max() / t.abs().max()) for g, t in zip(grads["hip"], grads["torch"]))
    fwd = _alternate({k: forward(k) for k in routes}, a.steps, a.warmup, a.repeats)
    both = _alternate({k: step(k) for k in routes}, a.steps, a.warmup, a.repeats)
    return {"N": n, "forward": _summary(fwd), "forward_backward": _summary(both),
            "bytes_per_row": {"forward": 12 + 4 + 4 + 12 + 4, "backward": 12 + 4 + 4 + 12 + 4 + 12 + 4},
            "worst_difference": difference, "worst_relative_gradient_difference": gradient_difference}


class _Camera:
    def __init__(self, cam, dev):
        t = lambda value: torch.tensor(value, dtype=torch.float32, device=dev)
        self.world_to_camera, self.full_projection, self.camera_center = (cam[k].to(dev) for k in ("world_to_camera", "full_projection", "camera_center"))
        self.fx, self.fy, self.cx, self.cy = t(cam["fx"]), t(cam["fy"]), t(cam["cx"]), t(cam["cy"])
        self.width, self.height = torch.tensor(cam["width"], dtype=torch.int32, device=dev), torch.tensor(cam["height"], dtype=torch.int32, device=dev)


class _Model:
    """What the plugins read of the reference's MipSplattingModel: raw scales and opacities behind exp / sigmoid getters, activated
    rotations, a filter."""

    def __init__(self, means, scales, quats, opac, shs, filter_3d, dev):
        leaf = lambda t: t.contiguous().to(dev).requires_grad_(True)
        self.properties = {"means": leaf(means), "scales": leaf(torch.log(scales)), "rotations": leaf(quats), "shs_dc": leaf(shs[:, :1]),
                           "shs_rest": leaf(shs[:, 1:]), "opacities": leaf(torch.logit(opac.reshape(-1, 1).clamp(1e-4, 1 - 1e-4)))}
        self.filter_3d = filter_3d.reshape(-1, 1).to(dev)
        self.config = types.SimpleNamespace(opacity_compensation=True)
        self.active_sh_degree, self.is_pre_activated = 3, False

    get_xyz = property(lambda s: s.properties["means"])

    def get_means(self): return self.properties["means"]
    def get_scales(self): return torch.exp(self.properties["scales"])
    def get_opacities(self): return torch.sigmoid(self.properties["opacities"])
    def get_rotations(self): return self.properties["rotations"]
    def get_shs_dc(self): return self.properties["shs_dc"]
    def get_shs_rest(self): return self.properties["shs_rest"]
    def get_3d_filter(self): return self.filter_3d


def measure_plugin(a, dev):
    from gspl_amd import mip, synthetic
    from gspl_amd.renderers import HipGSplatMipSplattingRendererV2, HipGSplatMipSplattingRendererV2Module

    class TorchMipModule(HipGSplatMipSplattingRendererV2Module):
        def get_scales(self, camera, gaussian_model, **kwargs):
            opacities, scales = torch_apply_3d_filter(gaussian_model.get_3d_filter(), gaussian_model.get_opacities(), gaussian_model.get_scales(),
                                                      gaussian_model.config.opacity_compensation)
            return scales, opacities.squeeze(-1)

    wl = synthetic.WORKLOADS[WORKLOAD]
    means, scales, quats, opac, shs = synthetic.scene(wl["n"], seed=42)
    camera = _Camera(synthetic.camera(wl["width"], wl["height"], wl["fx"]), dev)
    model = _Model(means, scales, quats, opac, shs, torch.zeros(wl["n"]), dev)
    model.filter_3d = mip.compute_3d_filter([camera], model).detach()
    bg = torch.zeros(3, device=dev)
    target = torch.rand(3, wl["height"], wl["width"], generator=torch.Generator().manual_seed(13)).to(dev)
    modules = {"torch": TorchMipModule(HipGSplatMipSplattingRendererV2()), "hip": HipGSplatMipSplattingRendererV2().instantiate()}

    def step(route):
        def run():
            for p in model.properties.values():
                p.grad = None
            (modules[route](camera, model, bg)["render"] - target).abs().mean().backward()
        return run
    images = {}
    with torch.no_grad():
        for k, module in modules.items():
            images[k] = module(camera, model, bg)["render"]
    times = _alternate({k: step(k) for k in modules}, a.steps, a.warmup, a.repeats)
    return {"workload": WORKLOAD, "N": wl["n"], "frame": [wl["height"], wl["width"]], "forward_backward": _summary(times),
            "worst_pixel_difference": float((images["hip"] - images["torch"]).abs().max())}


def cases():
    out = [(f"filter_{n}_{C}", "wall") for n in SIZES for C in CAMERAS]
    out += [(f"apply_{n}", what) for n in SIZES for what in ("forward", "forward_backward")]
    return out + [("plugin", "forward_backward")]


def verdict(runs):
    out = {}
    for case, what in cases():
        hip = [t for r in runs for t in r[case][what]["ms_repeats"]["hip"]]
        ref = [t for r in runs for t in r[case][what]["ms_repeats"]["torch"]]
        out[f"{case}_{what}"] = {"hip_ms_range": [min(hip), max(hip)], "torch_ms_range": [min(ref), max(ref)],
                                 "hip_faster_beyond_spread": max(hip) < min(ref)}
    out["runs"] = len(runs)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--time-limit", type=int, default=420)
    p.add_argument("--out", default=os.path.join(T.ROOT, "profiles", "mip_time.json"))
    a = p.parse_args()
    signal.alarm(a.time_limit)
    import gspl_amd  # noqa: F401
    assert torch.cuda.is_available(), "mip_time measures on the GPU"
    dev = torch.device("cuda:0")
    run = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    for n in SIZES:
        for C in CAMERAS:
            run[f"filter_{n}_{C}"] = measure_filter(n, C, a, dev)
        run[f"apply_{n}"] = measure_apply(n, a, dev)
        torch.cuda.empty_cache()
    run["plugin"] = measure_plugin(a, dev)
    signal.alarm(0)
    result = {"tool": "mip_time", "runs": []}
    if os.path.exists(a.out):
        with open(a.out) as f:
            previous = json.load(f)
        if previous.get("tool") == "mip_time":
            result["runs"] = previous.get("runs", [])
    result["runs"].append(run)
    result["verdict"] = verdict(result["runs"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"run": run, "verdict": result["verdict"]}))


if __name__ == "__main__":
    main()

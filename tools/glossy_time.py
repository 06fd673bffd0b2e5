"""The Glossy-Gaussian route's view-dependent opacity: `ops.sh_view_opacities` (csrc/glossy.hip) against the reference's formulation,
F.normalize -> `eval_sh_decomposed` + 0.5 -> clamp(0, 1) on [N, 1] tensors in float32 torch ops (restated below, degree 3), on the same
GPU, in one process, the two routes alternating repeat by repeat.

(a) The op alone at N = 100 000 and 1 000 000, degree 3, `opacity_rest` [N, 15, 1]: forward + backward into both parameters (gradients
    cleared per step, as autograd does; three rows in ten carry no gradient, as invisible Gaussians do), median of `--steps` samples
    per repeat; a sample runs the route as often as it takes to fill ~20 ms.  `forward` is the same without autograd.
(b) The plugin: `HipGlossyRenderer` on S-800-100k (100 000 Gaussians, 800 x 800), forward + backward of an L1 loss, against the same
    plugin with the torch expression in `get_opacities`.
`worst_difference`: the two routes' opacities, and their gradients relative to the largest gradient.  These are whole calls, host work
included; the kernels alone are not measured here.

Each run of this command APPENDS to `runs` in the output file; `verdict` is computed over every run in it: a route counts as faster
only where its slowest repeat of any run is below the other's fastest.  The process ends itself after `--time-limit` seconds.
  python tools/glossy_time.py [--steps 5] [--warmup 2] [--repeats 3] [--out profiles/glossy_time.json]"""
import argparse
import json
import math
import os
import signal
import statistics

import _step_time as T  # noqa: F401  (puts the repository root on sys.path)
import torch

SIZES = (100_000, 1_000_000)
DEGREE, KR = 3, 15
WORKLOAD = "S-800-100k"
C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)


def torch_view_opacities(means, camera_center, dc, rest):
    """`GlossyRendererModule.get_opacities` at degree 3, operation by operation as the reference's torch code has it."""
    d = torch.nn.functional.normalize(means.detach() - camera_center, dim=-1)
    result = C0 * dc[..., 0, :]
    x, y, z = d[..., 0:1], d[..., 1:2], d[..., 2:3]
    result = (result - C1 * y * rest[..., 0, :] + C1 * z * rest[..., 1, :] - C1 * x * rest[..., 2, :])
    xx, yy, zz = x * x, y * y, z * z
    xy, yz, xz = x * y, y * z, x * z
    result = (result + C2[0] * xy * rest[..., 3, :] + C2[1] * yz * rest[..., 4, :] + C2[2] * (2.0 * zz - xx - yy) * rest[..., 5, :] +
              C2[3] * xz * rest[..., 6, :] + C2[4] * (xx - yy) * rest[..., 7, :])
    result = (result + C3[0] * y * (3 * xx - yy) * rest[..., 8, :] + C3[1] * xy * z * rest[..., 9, :] +
              C3[2] * y * (4 * zz - xx - yy) * rest[..., 10, :] + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * rest[..., 11, :] +
              C3[4] * x * (4 * zz - xx - yy) * rest[..., 12, :] + C3[5] * z * (xx - yy) * rest[..., 13, :] +
              C3[6] * x * (xx - 3 * yy) * rest[..., 14, :])
    return torch.clamp((result + 0.5).squeeze(-1), min=0., max=1.)


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


def _alternate(routes, steps, warmup, repeats):
    times = {k: [] for k in routes}
    for rep in range(repeats):
        for k in (list(routes) if rep % 2 == 0 else list(routes)[::-1]):
            times[k].append(_median_ms(routes[k], steps, warmup))
    return times


def _summary(times):
    return {"ms_median_of_repeats": {k: round(statistics.median(v), 4) for k, v in times.items()},
            "ms_repeats": {k: [round(t, 4) for t in v] for k, v in times.items()}}


def measure_op(n, a, dev):
    from gspl_amd import ops
    gen = torch.Generator().manual_seed(11)
    means = (torch.rand(n, 3, generator=gen) * 2 - 1).to(dev)
    camera = torch.tensor([0.1, -0.2, 0.3], device=dev)
    dc = (1.5 * torch.randn(n, 1, 1, generator=gen)).to(dev).requires_grad_(True)
    rest = (0.5 * torch.randn(n, KR, 1, generator=gen)).to(dev).requires_grad_(True)
    v = (torch.randn(n, generator=gen) * (torch.rand(n, generator=gen) > 0.3)).to(dev)
    routes = {"torch": lambda: torch_view_opacities(means, camera, dc, rest), "hip": lambda: ops.sh_view_opacities(DEGREE, means, camera, dc, rest)}

    def forward(route):
        def run():
            with torch.no_grad():
                return routes[route]()
        return run

    def step(route):
        def run():
            dc.grad = rest.grad = None
            (routes[route]() * v).sum().backward()
        return run
    values, grads = {}, {}
    for k in routes:
        step(k)()
        values[k], grads[k] = forward(k)(), (dc.grad.clone(), rest.grad.clone())
    difference = float((values["hip"] - values["torch"]).abs().max())
    gradient_difference = max(float((g - t).abs().max() / t.abs().max()) for g, t in zip(grads["hip"], grads["torch"]))
    fwd = _alternate({k: forward(k) for k in routes}, a.steps, a.warmup, a.repeats)
    both = _alternate({k: step(k) for k in routes}, a.steps, a.warmup, a.repeats)
    return {"N": n, "degree": DEGREE, "opacity_rest_columns": KR, "zero_gradient_share": round(float((v == 0).float().mean()), 3),
            "clamped_share": round(float(((values["torch"] == 0) | (values["torch"] == 1)).float().mean()), 3),
            "forward": _summary(fwd), "forward_backward": _summary(both),
            "bytes_per_row": {"forward": 12 + 4 + 4 * KR + 4, "backward": 12 + 4 + 4 * KR + 4 + 4 + 4 * KR},
            "worst_difference": difference, "worst_relative_gradient_difference": gradient_difference}


class _Camera:
    def __init__(self, cam, dev):
        t = lambda value: torch.tensor(value, dtype=torch.float32, device=dev)
        self.world_to_camera, self.full_projection, self.camera_center = (cam[k].to(dev) for k in ("world_to_camera", "full_projection", "camera_center"))
        self.fx, self.fy, self.cx, self.cy = t(cam["fx"]), t(cam["fy"]), t(cam["cx"]), t(cam["cy"])
        self.width, self.height = torch.tensor(cam["width"], dtype=torch.int32, device=dev), torch.tensor(cam["height"], dtype=torch.int32, device=dev)


class _Model:
    """What the plugin reads of the reference's GlossyGaussianModel, with activated scales and rotations."""

    def __init__(self, means, scales, quats, opac, shs, rest, dev):
        leaf = lambda t: t.contiguous().to(dev).requires_grad_(True)
        self.properties = {"means": leaf(means), "scales": leaf(scales), "rotations": leaf(quats), "shs_dc": leaf(shs[:, :1]), "shs_rest": leaf(shs[:, 1:]),
                           "opacities": leaf((opac.reshape(-1, 1, 1) - 0.5) / C0), "opacity_rest": leaf(rest)}
        self.active_sh_degree, self.is_pre_activated = DEGREE, False

    get_xyz = property(lambda s: s.properties["means"])

    def get_means(self): return self.properties["means"]
    def get_scales(self): return self.properties["scales"]
    def get_rotations(self): return self.properties["rotations"]
    def get_shs_dc(self): return self.properties["shs_dc"]
    def get_shs_rest(self): return self.properties["shs_rest"]


def measure_plugin(a, dev):
    from gspl_amd import synthetic
    from gspl_amd.renderers import HipGlossyRenderer, HipGSplatV1Renderer, HipGSplatV1RendererModule

    class TorchGlossyModule(HipGSplatV1RendererModule):
        def get_opacities(self, camera, gaussian_model, projections, visibility_filter, status, **kwargs):
            p = gaussian_model.properties
            return torch_view_opacities(gaussian_model.get_xyz, camera.camera_center, p["opacities"], p["opacity_rest"]), status

    wl = synthetic.WORKLOADS[WORKLOAD]
    means, scales, quats, opac, shs = synthetic.scene(wl["n"], seed=42)
    gen = torch.Generator().manual_seed(13)
    model = _Model(means, scales, quats, opac, shs, 0.3 * torch.randn(wl["n"], KR, 1, generator=gen), dev)
    camera = _Camera(synthetic.camera(wl["width"], wl["height"], wl["fx"]), dev)
    bg = torch.zeros(3, device=dev)
    target = torch.rand(3, wl["height"], wl["width"], generator=gen).to(dev)
    modules = {"torch": TorchGlossyModule(HipGSplatV1Renderer()), "hip": HipGlossyRenderer().instantiate()}

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


def verdict(runs):
    out = {}
    cases = [(f"op_{n}", what) for n in SIZES for what in ("forward", "forward_backward")] + [("plugin", "forward_backward")]
    for case, what in cases:
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
    p.add_argument("--time-limit", type=int, default=300)
    p.add_argument("--out", default=os.path.join(T.ROOT, "profiles", "glossy_time.json"))
    a = p.parse_args()
    signal.alarm(a.time_limit)
    import gspl_amd  # noqa: F401
    assert torch.cuda.is_available(), "glossy_time measures on the GPU"
    dev = torch.device("cuda:0")
    run = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    for n in SIZES:
        run[f"op_{n}"] = measure_op(n, a, dev)
        torch.cuda.empty_cache()
    run["plugin"] = measure_plugin(a, dev)
    signal.alarm(0)
    result = {"tool": "glossy_time", "runs": []}
    if os.path.exists(a.out):
        with open(a.out) as f:
            previous = json.load(f)
        if previous.get("tool") == "glossy_time":
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

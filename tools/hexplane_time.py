"""The HexPlane field of the 4D-GS route: `ops.hexplane_encode` (csrc/hexplane.hip) against the field as the reference formulates it — six
`F.grid_sample` per level on channel-major [1, F, R_b, R_a] parameters, a product chain and a cat, in float32 torch ops — on the same
GPU, in one process, the two routes alternating repeat by repeat; and the `HipVanillaGS4DRenderer` frame against the reference's call
sequence on the same rasterizer.

(a) Forward alone (no autograd) and forward + backward (the gradient of every plane, cleared per step as autograd does), median of
    `--steps` runs per repeat, on 4DGaussians' D-NeRF setting ([64, 64, 64, 25], multires [1, 2], F = 32) at N = 100 k and its
    DyNeRF-sized setting ([64, 64, 64, 150], multires [1, 2, 4, 8], F = 32) at N = 1 M; points uniform in 1.3 x the box, one time per
    call.  The HIP forward + backward is timed twice: with the packed table as the leaf, and from the reference-shaped parameters
    (`hexplane_pack` and its backward inside the step).  `achieved_TBs` is the algorithmic traffic (24 corner rows + the output row per
    point and level) over the forward's time; `peak_MiB` the allocator's peak above what was allocated before the route ran.
(b) One viewer frame (no autograd) on S-800-100k-shaped Gaussians: the plugin, and the reference's sequence — the positional embeddings
    it computes and does not read, the repeated time column, the torch field, the same MLPs, the same `HipVanillaRenderer.render`.

Each run of this command APPENDS to `runs` in the output file; `verdict` is computed over every run in it (the spread comes from
repeating the identical command): the HIP forward counts as faster only where its slowest repeat of any run is below the torch
formulation's fastest.  The process ends itself after `--time-limit` seconds.
  python tools/hexplane_time.py [--steps 5] [--warmup 2] [--repeats 3] [--out profiles/hexplane_time.json]"""
import argparse
import itertools
import json
import os
import signal
import statistics
import tempfile
import types
from argparse import Namespace

import _step_time as T  # noqa: F401  (puts the repository root on sys.path)
import torch
import torch.nn.functional as F

PLANES = list(itertools.combinations(range(4), 2))
SETTINGS = (("dnerf_N_100k", [64, 64, 64, 25], [1, 2], 100_000), ("dynerf_N_1M", [64, 64, 64, 150], [1, 2, 4, 8], 1_000_000))


def _median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    events = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        events.append((e0, e1))
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in events)


def _peak_mib(fn):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def torch_field(x, time, planes, aabb):
    """The reference's formulation: normalise, append the time column, 6 grid_sample per level, product, cat."""
    pts = (x - aabb[0]) * (2.0 / (aabb[1] - aabb[0])) - 1.0
    pts = torch.cat((pts, time), dim=-1)
    levels = []
    for grids in planes:
        product = 1.0
        for grid, (a, b) in zip(grids, PLANES):
            sample = F.grid_sample(grid, pts[..., [a, b]].view(1, 1, -1, 2), align_corners=True, mode="bilinear", padding_mode="border")
            product = product * sample.view(grid.shape[1], -1).transpose(-1, -2)
        levels.append(product)
    return torch.cat(levels, dim=-1)


def _alternate(routes, steps, warmup, repeats):
    times = {k: [] for k in routes}
    for rep in range(repeats):
        for k in (list(routes) if rep % 2 == 0 else list(routes)[::-1]):
            times[k].append(_median_ms(routes[k], steps, warmup))
    return times


def _summary(times):
    return {"ms_median_of_repeats": {k: round(statistics.median(v), 4) for k, v in times.items()},
            "ms_repeats": {k: [round(t, 4) for t in v] for k, v in times.items()}}


def measure_field(name, resolution, multires, N, a, dev):
    from gspl_amd import ops
    lay = ops.hexplane_layout(resolution, multires, 32)
    gen = torch.Generator().manual_seed(42)
    planes = [[(0.1 + 0.4 * torch.rand(lay.plane_shape(level, p), generator=gen)).to(dev) for p in range(6)] for level in range(lay.n_levels)]
    aabb = torch.tensor([[1.6] * 3, [-1.6] * 3], device=dev)
    box = ops.hexplane_box(aabb)
    x = ((torch.rand(N, 3, generator=gen) * 2 - 1) * 1.6 * 1.3).to(dev)
    v_out = torch.randn(N, lay.n_output_dims, generator=gen).to(dev)
    time, time_column = 0.4375, torch.full((N, 1), 0.4375, device=dev)
    table = ops.hexplane_pack(planes, lay).contiguous()
    with torch.no_grad():
        difference = float((ops.hexplane_forward(x, time, table, box, lay) - torch_field(x, time_column, planes, aabb)).abs().max())

    def torch_forward():
        with torch.no_grad():
            return torch_field(x, time_column, planes, aabb)

    def hip_forward():
        return ops.hexplane_forward(x, time, table, box, lay)
    leaves = [[p.detach().clone().requires_grad_(True) for p in level] for level in planes]
    flat = [p for level in leaves for p in level]
    table_leaf = table.detach().clone().requires_grad_(True)

    def torch_step():
        for p in flat:
            p.grad = None
        torch_field(x, time_column, leaves, aabb).backward(v_out)

    def hip_step_table():
        table_leaf.grad = None
        ops.hexplane_encode(x, time, table_leaf, box, lay).backward(v_out)

    def hip_step_planes():
        for p in flat:
            p.grad = None
        ops.hexplane_encode(x, time, ops.hexplane_pack(leaves, lay), box, lay).backward(v_out)
    forward = _alternate({"torch": torch_forward, "hip": hip_forward}, a.steps, a.warmup, a.repeats)
    step = _alternate({"torch": torch_step, "hip_table_leaf": hip_step_table, "hip_from_planes": hip_step_planes}, a.steps, a.warmup, a.repeats)
    traffic = N * lay.n_levels * (24 + 1) * 32 * 4
    hip_ms = statistics.median(forward["hip"])
    return {"resolution": resolution, "multires": multires, "features": 32, "points": N, "table_rows": lay.total, "table_MiB": round(lay.n_params * 4 / 2 ** 20, 1),
            "forward": _summary(forward), "forward_backward": _summary(step),
            "forward_speedup": round(statistics.median(forward["torch"]) / hip_ms, 2),
            "forward_backward_speedup_table_leaf": round(statistics.median(step["torch"]) / statistics.median(step["hip_table_leaf"]), 2),
            "forward_backward_speedup_from_planes": round(statistics.median(step["torch"]) / statistics.median(step["hip_from_planes"]), 2),
            "algorithmic_bytes": traffic, "achieved_TBs": {k: round(traffic / (statistics.median(v) * 1e-3) / 1e12, 4) for k, v in forward.items()},
            "peak_MiB": {"torch_forward": _peak_mib(torch_forward), "hip_forward": _peak_mib(hip_forward), "torch_forward_backward": _peak_mib(torch_step),
                         "hip_forward_backward_table_leaf": _peak_mib(hip_step_table), "hip_forward_backward_from_planes": _peak_mib(hip_step_planes)},
            "worst_forward_difference": difference}


def measure_frame(a, dev):
    """The plugin's frame against the reference's call sequence, D-NeRF arguments, one model directory written for the run."""
    from gspl_amd import synthetic
    from gspl_amd.gs4d import HipDeformNetwork, frequency_embedding
    from gspl_amd.renderers import HipVanillaGS4DRenderer, HipVanillaRenderer
    args = Namespace(net_width=64, timebase_pe=4, defor_depth=1, posebase_pe=10, scale_rotation_pe=2, opacity_pe=2, timenet_width=64,
                     timenet_output=32, bounds=1.6, grid_pe=0, multires=[1, 2], no_dx=False, no_grid=False, no_ds=False, no_dr=False, no_do=True,
                     no_dshs=True, empty_voxel=False, static_mlp=False, apply_rotation=False,
                     kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 32, "resolution": [64, 64, 64, 25]})
    wl = synthetic.WORKLOADS[a.workload]
    W, H = wl["width"], wl["height"]
    means, scales, quats, opac, shs = T.scene(wl, dev)
    with tempfile.TemporaryDirectory() as root:
        torch.manual_seed(3)
        net = HipDeformNetwork(args)
        with torch.no_grad():
            for head in (net.deformation_net.pos_deform, net.deformation_net.scales_deform, net.deformation_net.rotations_deform):
                head[3].weight.mul_(0.02)          # small deformations: the frame keeps the workload's shape
        ckpt = os.path.join(root, "point_cloud", "iteration_1")
        os.makedirs(ckpt)
        with open(os.path.join(root, "cfg_args"), "w") as f:
            f.write(repr(args))
        torch.save(net.state_dict(), os.path.join(ckpt, "deformation.pth"))
        torch.save(torch.ones(means.shape[0], dtype=torch.bool), os.path.join(ckpt, "deformation_table.pth"))
        renderer = HipVanillaGS4DRenderer(root, 1, dev)
    pc = types.SimpleNamespace(get_xyz=means, scales=torch.log(scales), rotations=quats, opacities=torch.logit(opac.clamp(1e-4, 1 - 1e-4)),
                               get_features=shs, active_sh_degree=3, scale_activation=torch.exp, opacity_activation=torch.sigmoid,
                               rotation_activation=F.normalize)
    cam = synthetic.CameraObject(synthetic.camera(W, H, wl["fx"]), dev)
    cam.time = torch.tensor(0.4375, device=dev)
    bg = torch.zeros(3, device=dev)
    net = renderer.deformation
    deform, field = net.deformation_net, net.deformation_net.grid

    def reference_frame():
        with torch.no_grad():
            time = cam.time.repeat(means.shape[0], 1)
            point_emb = frequency_embedding(pc.get_xyz, net.pos_poc)
            scales_emb = frequency_embedding(pc.scales, net.rotation_scaling_poc)
            rotations_emb = frequency_embedding(pc.rotations, net.rotation_scaling_poc)
            hidden = deform.feature_out(torch_field(point_emb[:, :3], time[:, :1], [list(level) for level in field.grids], field.aabb))
            mask = torch.ones_like(pc.opacities[:, 0]).unsqueeze(-1)
            new_means = point_emb[:, :3] * mask + deform.pos_deform(hidden)
            new_scales = scales_emb[:, :3] * mask + deform.scales_deform(hidden)
            new_rotations = rotations_emb[:, :4] + deform.rotations_deform(hidden)
            return HipVanillaRenderer.render(means3D=new_means, opacity=pc.opacity_activation(pc.opacities), scales=pc.scale_activation(new_scales),
                                             rotations=pc.rotation_activation(new_rotations), features=pc.get_features, active_sh_degree=3,
                                             viewpoint_camera=cam, bg_color=bg, scaling_modifier=1.0)["render"]

    def plugin_frame():
        with torch.no_grad():
            return renderer(cam, pc, bg)["render"]

    def vanilla_frame():
        with torch.no_grad():
            return HipVanillaRenderer.render(means3D=means, opacity=opac, scales=scales, rotations=quats, features=shs, active_sh_degree=3,
                                             viewpoint_camera=cam, bg_color=bg, scaling_modifier=1.0)["render"]
    difference = float((plugin_frame() - reference_frame()).abs().max())
    times = _alternate({"reference_sequence": reference_frame, "plugin": plugin_frame, "rasterizer_alone": vanilla_frame}, max(a.steps, 10), a.warmup + 2, a.repeats)
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"workload": a.workload, "n": wl["n"], "width": W, "height": H, **_summary(times),
            "reference_over_plugin": round(med["reference_sequence"] / med["plugin"], 2), "worst_image_difference": difference,
            "peak_MiB": {"reference_sequence": _peak_mib(reference_frame), "plugin": _peak_mib(plugin_frame)}}


def verdict(runs):
    out = {}
    for name, *_ in SETTINGS:
        hip = [t for r in runs for t in r[name]["forward"]["ms_repeats"]["hip"]]
        ref = [t for r in runs for t in r[name]["forward"]["ms_repeats"]["torch"]]
        out[name] = {"hip_forward_ms_range": [min(hip), max(hip)], "torch_forward_ms_range": [min(ref), max(ref)],
                     "hip_forward_faster_beyond_spread": max(hip) < min(ref)}
    out["runs"] = len(runs)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--workload", default="S-800-100k")
    p.add_argument("--time-limit", type=int, default=540)
    p.add_argument("--out", default=os.path.join(T.ROOT, "profiles", "hexplane_time.json"))
    a = p.parse_args()
    signal.alarm(a.time_limit)
    import gspl_amd  # noqa: F401
    assert torch.cuda.is_available(), "hexplane_time measures on the GPU"
    dev = torch.device("cuda:0")
    run = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    for name, resolution, multires, N in SETTINGS:
        run[name] = measure_field(name, resolution, multires, N, a, dev)
        torch.cuda.empty_cache()
    run["viewer_frame"] = measure_frame(a, dev)
    signal.alarm(0)
    result = {"tool": "hexplane_time", "runs": []}
    if os.path.exists(a.out):
        with open(a.out) as f:
            previous = json.load(f)
        if previous.get("tool") == "hexplane_time":
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

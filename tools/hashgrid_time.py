"""The grid encoding of the SWAG route: `ops.hashgrid_encode` (csrc/hashgrid.hip) against the same encoding written with float32 torch
ops — index arithmetic, a gather per corner, `index_add_` per corner in the backward — on the same GPU, in one process, the two
routes alternating repeat by repeat; and the `HipSWAGRenderer` step against `HipVanillaRenderer`'s.

(a) SWAG's defaults (12 levels, 4 features, 2^19 rows per hashed level, base 16, max 2048; 4 500 336 rows, 72 MB), points uniform
    in [0, 1]^3: N = 1 M with 30 % non-zero rows of v_out (what a frame that blends 30 % of the Gaussians leaves), and N = 100 k with
    every row.  Forward + backward (the table's gradient, cleared per step as autograd does), median of `--steps` runs per repeat.
(b) The backward launch alone, into a buffer that is not cleared, for the atomic sizing: `atomic_bytes` = non-zero rows x levels x 8
    corners x 16 B is what the launch would add without the in-wave sum of equal destinations, `implied_atomic_TBs` that figure over the
    launch's time, against the 1.3 TB/s chip-wide rate of well-shaped float atomics.  Also with the points sorted by their level-3 cell
    (a spatially coherent order), where consecutive points share destinations at the dense levels.
(c) One training step (forward, L1 loss, backward) on S-800-100k with the plugin and with `HipVanillaRenderer` on the same model.

The process ends itself after `--time-limit` seconds.
  python tools/hashgrid_time.py [--steps 5] [--warmup 2] [--repeats 3] [--out profiles/hashgrid_time.json]"""
import argparse
import json
import math
import os
import signal
import statistics
import types

import _step_time as T  # noqa: F401  (puts the repository root on sys.path)
import torch

PRIMES = (1, 2654435761, 805459861)


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


def torch_route(x, table, lv, v_out):
    """Forward and the table's gradient with float32 torch ops; -> (out, v_table)."""
    F, L = lv.n_features_per_level, lv.n_levels
    out = torch.empty((x.shape[0], L * F), dtype=torch.float32, device=x.device)
    v_table = torch.zeros_like(table)
    for level in range(L):
        pos = x * float(lv.scales[level]) + 0.5
        floor = torch.floor(pos)
        frac, cell = pos - floor, floor.to(torch.int64) & 0xFFFFFFFF
        res, size, first = int(lv.resolutions[level]), int(lv.sizes[level]), int(lv.offsets[level])
        acc = torch.zeros((x.shape[0], F), dtype=torch.float32, device=x.device)
        g = v_out[:, level * F:(level + 1) * F]
        for corner in range(8):
            w, index = None, torch.zeros_like(cell[:, 0])
            for d in range(3):
                bit = (corner >> d) & 1
                c = (cell[:, d] + bit) & 0xFFFFFFFF
                index = (index ^ ((c * PRIMES[d]) & 0xFFFFFFFF)) if lv.hashed[level] else ((index + c * (res ** d)) & 0xFFFFFFFF)
                factor = frac[:, d] if bit else 1 - frac[:, d]
                w = factor if w is None else w * factor
            rows = first + index % size
            acc += w[:, None] * table[rows]
            v_table.index_add_(0, rows, w[:, None] * g)
        out[:, level * F:(level + 1) * F] = acc
    return out, v_table


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--workload", default="S-800-100k")
    p.add_argument("--time-limit", type=int, default=540)
    p.add_argument("--out", default=os.path.join(T.ROOT, "profiles", "hashgrid_time.json"))
    a = p.parse_args()
    signal.alarm(a.time_limit)
    import gspl_amd  # noqa: F401
    from gspl_amd import ops, swag, synthetic
    from gspl_amd.renderers import HipSWAGRenderer, HipVanillaRenderer
    assert torch.cuda.is_available(), "hashgrid_time measures on the GPU"
    dev = torch.device("cuda:0")
    lv = ops.hashgrid_levels(3, 12, 4, 19, 16, math.exp((math.log(2048) - math.log(16)) / 11))
    table = (ops.hashgrid_table(lv, 1337, dev) * 1e4).reshape(lv.total, 4)
    result = {"tool": "hashgrid_time", "device": torch.cuda.get_device_name(0), "levels": 12, "features_per_level": 4, "table_rows": lv.total,
              "table_bytes": lv.n_params * 4, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "guide_atomic_rate_TBs": 1.3}
    gen = torch.Generator().manual_seed(42)
    for name, N, share in (("N_1M_30pct_rows", 1_000_000, 0.3), ("N_100k_all_rows", 100_000, 1.0)):
        x = torch.rand(N, 3, generator=gen).to(dev)
        v_out = torch.randn(N, 48, generator=gen)
        if share < 1:
            v_out[torch.rand(N, generator=gen) >= share] = 0
        v_out = v_out.to(dev)
        nonzero_rows = int((v_out != 0).any(dim=1).sum())
        leaf = table.detach().clone().requires_grad_(True)

        def kernel():
            leaf.grad = None
            out = ops.hashgrid_encode(x, leaf, lv)
            out.backward(v_out)
            return out, leaf.grad

        def restated():
            return torch_route(x, table, lv, v_out)

        (ok, gk), (orr, gr) = kernel(), restated()
        worst_out = float((ok.detach() - orr).abs().max() / orr.abs().max())
        worst_grad = float((gk - gr).abs().max() / gr.abs().max())
        del ok, gk, orr, gr
        routes = {"torch": restated, "hip": kernel}
        medians = {k: [] for k in routes}
        for rep in range(a.repeats):
            for k in (list(routes) if rep % 2 == 0 else list(routes)[::-1]):
                medians[k].append(_median_ms(routes[k], a.steps, a.warmup))
        med = {k: statistics.median(v) for k, v in medians.items()}
        # the launches alone
        buffer = torch.zeros_like(table)
        fwd_ms = _median_ms(lambda: ops.hashgrid_forward(x, table, lv), a.steps, a.warmup)
        bwd_ms = _median_ms(lambda: ops.hashgrid_backward(x, table, lv, v_out, buffer), a.steps, a.warmup)
        cell = torch.floor(x * float(lv.scales[3]) + 0.5).to(torch.int64)
        order = torch.argsort((cell[:, 2] * 64 + cell[:, 1]) * 64 + cell[:, 0])
        xs, vs = x[order].contiguous(), v_out[order].contiguous()
        bwd_sorted_ms = _median_ms(lambda: ops.hashgrid_backward(xs, table, lv, vs, buffer), a.steps, a.warmup)
        atomic_bytes = nonzero_rows * 12 * 8 * 16
        result[name] = {
            "points": N, "nonzero_v_out_rows": nonzero_rows,
            "fwd_bwd_ms_median_of_repeats": {k: round(v, 4) for k, v in med.items()},
            "fwd_bwd_ms_repeats": {k: [round(t, 4) for t in v] for k, v in medians.items()},
            "speedup": round(med["torch"] / med["hip"], 2), "hip_below_torch": med["hip"] < med["torch"],
            "hip_faster_beyond_spread": max(medians["hip"]) < min(medians["torch"]),
            "fwd_launch_ms": round(fwd_ms, 4), "bwd_launch_ms": round(bwd_ms, 4), "bwd_launch_cell_sorted_ms": round(bwd_sorted_ms, 4),
            "atomic_bytes": atomic_bytes, "implied_atomic_TBs": round(atomic_bytes / (bwd_ms * 1e-3) / 1e12, 4),
            "implied_atomic_TBs_cell_sorted": round(atomic_bytes / (bwd_sorted_ms * 1e-3) / 1e12, 4),
            "fraction_of_guide_rate": round(atomic_bytes / (bwd_ms * 1e-3) / 1.3e12, 4),
            "worst_out_difference_over_max": worst_out, "worst_gradient_difference_over_max": worst_grad,
        }
        del x, v_out, xs, vs, buffer, leaf

    # (c) the plugin's step against the vanilla plugin's, one model
    wl = synthetic.WORKLOADS[a.workload]
    W, H = wl["width"], wl["height"]
    means, scales, quats, opac, shs = T.scene(wl, dev)
    P = lambda t: t.clone().requires_grad_(True)
    model = types.SimpleNamespace(get_xyz=P(means), get_scaling=P(scales), get_rotation=P(quats), get_opacity=P(opac), get_features=P(shs),
                                  active_sh_degree=3, max_sh_degree=3, is_pre_activated=True)
    leaves = [model.get_xyz, model.get_scaling, model.get_rotation, model.get_opacity, model.get_features]
    cam = synthetic.camera(W, H, wl["fx"])
    camera = types.SimpleNamespace(
        world_to_camera=cam["world_to_camera"].to(dev), full_projection=cam["full_projection"].to(dev), camera_center=cam["camera_center"].to(dev),
        width=torch.tensor(W, device=dev), height=torch.tensor(H, device=dev), fov_x=torch.tensor(2 * math.atan(cam["tanfovx"]), device=dev),
        fov_y=torch.tensor(2 * math.atan(cam["tanfovy"]), device=dev), appearance_id=3)
    bg = torch.zeros(3, device=dev)
    target = torch.rand(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    swag_renderer = HipSWAGRenderer()
    swag_renderer.setup("fit", xyz=means)
    swag_renderer.to(dev)
    swag_renderer.training_setup(None)
    with torch.no_grad():
        swag_renderer.swag_model.grid_encoding.params.mul_(1e4)
    swag_leaves = leaves + list(swag_renderer.swag_model.parameters())
    vanilla = HipVanillaRenderer()

    def step(which):
        for leaf in swag_leaves:
            leaf.grad = None
        out = swag_renderer.training_forward(0, None, camera, model, bg) if which == "swag" else vanilla(camera, model, bg)
        (out["render"] - target).abs().mean().backward()

    times = {k: [] for k in ("vanilla", "swag")}
    for rep in range(a.repeats):
        for k in (list(times) if rep % 2 == 0 else list(times)[::-1]):
            times[k].append(_median_ms(lambda: step(k), max(a.steps, 10), a.warmup + 2))
    med = {k: statistics.median(v) for k, v in times.items()}
    result["plugin_step"] = {"workload": a.workload, "n": wl["n"], "width": W, "height": H,
                             "ms_per_step_median_of_repeats": {k: round(v, 4) for k, v in med.items()},
                             "ms_per_step_repeats": {k: [round(t, 4) for t in v] for k, v in times.items()},
                             "swag_over_vanilla": round(med["swag"] / med["vanilla"], 3),
                             "note": "forward, L1, backward; no optimizer step; the swag step includes clearing the 72 MB table gradient"}
    signal.alarm(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

"""The share of Gaussians whose Adam moments have ever moved (`exp_avg_sq != 0` in any column of `shs_rest`): the rows
`selective_adam_kernel` cannot pass over (csrc/adam.hip).  Two figures, one JSON line:

  default_line           bench.py's default step (S-1080p-1M, heterogeneous set, photometric loss, FusedAdam) after warm-up + timed steps
  reference_shaped_loop  the end of bench.py's reference-shaped loop (N changes, one opacity reset, the SH degree raised twice)

usage (on the GPU box): python tools/adam_live_rows.py [--workload S-1080p-1M] [--steps 200] [--warmup 20] [--loop-steps 450]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def live_share(optimizers):
    """(rows with a non-zero second moment in shs_rest, rows) over the optimizers' "shs_rest" group."""
    for opt in optimizers:
        for group in opt.param_groups:
            if group.get("name") == "shs_rest":
                v = opt.state[group["params"][0]]["exp_avg_sq"]
                return int((v.reshape(v.shape[0], -1) != 0).any(dim=1).sum()), int(v.shape[0])
    raise RuntimeError("no shs_rest group")


def default_line(a, dev):
    import bench
    import gspl_amd  # noqa: F401
    from gspl_amd import synthetic
    from gspl_amd.optimizers import FusedAdam
    wl = synthetic.WORKLOADS[a.workload]
    means, scales, quats, opac, shs = synthetic.workload_scene(wl, seed=42)
    cam_dicts = synthetic.camera_set(wl["width"], wl["height"], wl["fx"], count=16, distance=wl.get("distance", 4.0), kind="heterogeneous")
    stream = synthetic.ViewStream(16, shuffled=True, seed=42)
    tensors = [t.contiguous().to(dev).requires_grad_(True) for t in (means, scales, quats, opac, shs[:, :1], shs[:, 1:])]
    step = bench.make_step("vanilla", dev, wl, cam_dicts, tensors, "photometric", 0, 1, stream=stream)
    lrs = (1.6e-4, 5e-3, 1e-3, 5e-2, 2.5e-3, 2.5e-3 / 20.0)
    names = ("means", "scales", "rotations", "opacities", "shs_dc", "shs_rest")
    opt = FusedAdam([{"params": [t], "lr": lr * 1e-3, "name": n} for t, lr, n in zip(tensors, lrs, names)], eps=1e-15)
    stats = tuple(torch.zeros(wl["n"], device=dev) for _ in range(3))
    step.state["stats_buffers"] = stats
    shares = {}
    for k in range(1, a.warmup + a.steps + 1):
        st = step()
        with torch.no_grad():
            bench.densification_stats(st, *stats)
            opt.step()
        if k in (1, 16, a.warmup, a.warmup + a.steps):
            shares[k] = live_share([opt])
    return {"workload": a.workload, "live_rows_after_step": {k: {"live": s[0], "n": s[1], "share": round(s[0] / s[1], 4)} for k, s in shares.items()}}


def loop(a, dev):
    import bench
    import bench_loop as BL
    from gspl_amd import synthetic
    wl = synthetic.WORKLOADS[a.workload]
    cam_dicts = synthetic.camera_set(wl["width"], wl["height"], wl["fx"], count=16, distance=wl.get("distance", 4.0), kind="heterogeneous")
    seen, run = [], BL.run

    def recording_run(renderer, model, controller, optimizers, *args, **kw):
        seen[:] = [optimizers]
        return run(renderer, model, controller, optimizers, *args, **kw)
    BL.run = recording_run
    try:
        res = bench.reference_shaped_loop(dev, wl, cam_dicts, a.loop_steps, view_stream=synthetic.ViewStream(16, shuffled=True, seed=42))
    finally:
        BL.run = run
    live, n = live_share(seen[0])
    return {"steps": a.loop_steps, "n_start": res["n_start"], "n_end": res["n_end"], "live": live, "n": n, "share": round(live / n, 4),
            "events": len(res["events"])}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--workload", default="S-1080p-1M")
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--loop-steps", type=int, default=450)
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    print(json.dumps({"default_line": default_line(a, dev), "reference_shaped_loop": loop(a, dev) if a.loop_steps > 0 else None}))


if __name__ == "__main__":
    main()

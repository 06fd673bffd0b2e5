"""The SpotLess route outside the rasterizer: `gspl_amd.spotless.predict_mask` (csrc/spotless.hip) against `mlp_mask` as the reference
formulates it — a bilinear resampling of the [1280, 50, 50] feature map to the mask size, a cat with the 80-channel positional
encoding (computed over the whole grid every step, as the reference does), a permute into [pixels, 1360], Linear(1360, 16) -> ReLU -> Linear(16, 1) ->
Sigmoid and the resampling to the frame, in float32 torch ops — on the same GPU, in one process, the two routes alternating repeat by
repeat; and the reference's running-statistics update (the error map copied to the host, a 10 000-bin `torch.histogram` there)
against `ops.spotless_error_stats` + `RunningErrorStats.update`.

(a) Mask sizes 400 and 800 on a 1080p frame (1080 x 1920: both take the resizing branch).  Forward alone (no autograd), and forward +
    backward of the spot loss into the four parameters (gradients cleared per step, as autograd does), median of `--steps` samples per
    repeat; a sample runs the route as often as it takes to fill ~20 ms.  `peak_MiB` is the allocator's peak above what was allocated
    before the route ran.  `worst_difference` compares the two masks (the positional encoding is formed by the same operations on both sides).
(b) The statistics update on the same frame: per step, `render` and `gt` [3, 1080, 1920] on the device -> the histogram folded into
    the running one and the three thresholds.  The device route also writes the error map and both robust masks, which the reference
    computes elsewhere.

Each run of this command APPENDS to `runs` in the output file; `verdict` is computed over every run in it: a route counts as faster
only where its slowest repeat of any run is below the other's fastest.  The process ends itself after `--time-limit` seconds.
  python tools/spotless_time.py [--steps 5] [--warmup 2] [--repeats 3] [--out profiles/spotless_time.json]"""
import argparse
import json
import math
import os
import signal
import statistics
import types

import _step_time as T  # noqa: F401  (puts the repository root on sys.path)
import torch
import torch.nn.functional as F

C, H0, W0, H, W, BINS = 1280, 50, 50, 1080, 1920, 10000
MASK_SIZES = (400, 800)


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


def _peak_mib(fn):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def _alternate(routes, steps, warmup, repeats):
    times = {k: [] for k in routes}
    for rep in range(repeats):
        for k in (list(routes) if rep % 2 == 0 else list(routes)[::-1]):
            times[k].append(_median_ms(routes[k], steps, warmup))
    return times


def _summary(times):
    return {"ms_median_of_repeats": {k: round(statistics.median(v), 4) for k, v in times.items()},
            "ms_repeats": {k: [round(t, 4) for t in v] for k, v in times.items()}}


def dense_encoding(size, device):
    """The [80, size, size] positional encoding the reference builds every step, at its cost: the project's own axis encoding
    (gspl_amd.spotless.encode_coordinate) applied to the two full coordinate grids, not to the two axes."""
    from gspl_amd.spotless import axis_coordinate, encode_coordinate
    coord = axis_coordinate(size, device)
    rows, columns = coord[:, None].expand(size, size), coord[None, :].expand(size, size)
    return torch.cat([encode_coordinate(rows), encode_coordinate(columns)], dim=-1).permute(2, 0, 1)


def reference_mask(module, sf, height, width, size):
    """`mlp_mask`'s prediction in the reference's formulation (the resizing branch: max(height, width) > size) -> [height, width]."""
    dense = torch.cat([F.interpolate(sf[None], size=(size, size), mode="bilinear")[0], dense_encoding(size, sf.device)], dim=0)
    pred = module.mlp(dense.reshape(dense.shape[0], -1).permute(1, 0))
    return F.interpolate(pred.reshape(1, 1, size, size), size=(height, width), mode="bilinear")[0, 0]


def spot_loss(pred, upper, lower):
    return torch.mean(torch.relu(pred.flatten() - upper.flatten()) + torch.relu(lower.flatten() - pred.flatten()))


def measure_mask(size, a, dev):
    from gspl_amd import spotless
    torch.manual_seed(7)
    gen = torch.Generator().manual_seed(7)
    mlp = torch.nn.Sequential(torch.nn.Linear(C + 80, 16), torch.nn.ReLU(), torch.nn.Linear(16, 1), torch.nn.Sigmoid()).to(dev)
    module = types.SimpleNamespace(mlp=mlp)
    sf = torch.randn(C, H0, W0, generator=gen).to(dev)
    lower = (torch.rand(H, W, generator=gen) > 0.6).float().to(dev)
    upper = torch.maximum(lower, (torch.rand(H, W, generator=gen) > 0.5).float().to(dev))       # the two masks disagree on about a fifth
    with torch.no_grad():
        difference = float((spotless.predict_mask(module, sf, H, W, size)[1].reshape(H, W) - reference_mask(module, sf, H, W, size)).abs().max())

    def torch_forward():
        with torch.no_grad():
            return reference_mask(module, sf, H, W, size)

    def hip_forward():
        with torch.no_grad():
            return spotless.predict_mask(module, sf, H, W, size)[1]

    def torch_step():
        mlp.zero_grad(set_to_none=True)
        spot_loss(reference_mask(module, sf, H, W, size), upper, lower).backward()

    def hip_step():
        mlp.zero_grad(set_to_none=True)
        spot_loss(spotless.predict_mask(module, sf, H, W, size)[0], upper, lower).backward()
    torch_step()
    theirs = [p.grad.clone() for p in mlp.parameters()]
    hip_step()
    gradient_difference = max(float((p.grad - g).abs().max() / g.abs().max()) for p, g in zip(mlp.parameters(), theirs))
    forward = _alternate({"torch": torch_forward, "hip": hip_forward}, a.steps, a.warmup, a.repeats)
    step = _alternate({"torch": torch_step, "hip": hip_step}, a.steps, a.warmup, a.repeats)
    return {"mask_size": size, "frame": [H, W], "features": [C, H0, W0], "zero_gradient_share": round(float((upper != lower).float().mean()), 3),
            "forward": _summary(forward), "forward_backward": _summary(step),
            "forward_speedup": round(statistics.median(forward["torch"]) / statistics.median(forward["hip"]), 1),
            "forward_backward_speedup": round(statistics.median(step["torch"]) / statistics.median(step["hip"]), 1),
            "peak_MiB": {"torch_forward": _peak_mib(torch_forward), "hip_forward": _peak_mib(hip_forward),
                         "torch_forward_backward": _peak_mib(torch_step), "hip_forward_backward": _peak_mib(hip_step)},
            "worst_difference": difference, "worst_relative_gradient_difference": gradient_difference}


def measure_stats(a, dev):
    from gspl_amd import ops, spotless
    gen = torch.Generator().manual_seed(9)
    gt = torch.rand(3, H, W, generator=gen).to(dev)
    render = (gt + 0.2 * torch.randn(3, H, W, generator=gen).to(dev) * (torch.rand(1, H, W, generator=gen).to(dev) > 0.5)).clamp(0, 1)
    state = types.SimpleNamespace(hist=torch.zeros(BINS, device=dev), avg=torch.tensor(1., device=dev), lower=torch.tensor(0., device=dev),
                                  upper=torch.tensor(1., device=dev))
    stats = spotless.RunningErrorStats(bins=BINS, device=dev)

    def reference_update():
        """The reference's formulation: the error map to the host, the histogram there, every threshold through a boolean search."""
        err = (render - gt).abs().permute(1, 2, 0).mean(dim=-1)
        counts = torch.histogram(err.clone().cpu(), bins=BINS, range=(0.0, 1.0))[0].to(dev)
        state.hist.copy_(0.95 * state.hist + counts)
        for name, q in (("avg", 0.7), ("lower", 0.5), ("upper", 0.9)):
            reached = torch.cumsum(state.hist, 0) >= torch.sum(state.hist) * q
            getattr(state, name).fill_(torch.linspace(0, 1, BINS + 1)[torch.where(reached)[0][0]])

    def device_update():
        stats.update(ops.spotless_error_stats(render, gt, stats.thresholds, BINS)[1])
    reference_update(), device_update()
    same = [float(state.avg) == float(stats.avg), float(state.lower) == float(stats.lower), float(state.upper) == float(stats.upper)]
    hist_difference = float((state.hist - stats.hist).abs().max())
    times = _alternate({"reference": reference_update, "device": device_update}, a.steps, a.warmup, a.repeats)
    return {"frame": [H, W], "bins": BINS, **_summary(times),
            "speedup": round(statistics.median(times["reference"]) / statistics.median(times["device"]), 1),
            "peak_MiB": {"reference": _peak_mib(reference_update), "device": _peak_mib(device_update)},
            "same_thresholds_after_one_step": same, "worst_histogram_difference_after_one_step": hist_difference}


def verdict(runs):
    out = {}
    for size in MASK_SIZES:
        for what in ("forward", "forward_backward"):
            hip = [t for r in runs for t in r[f"mask_{size}"][what]["ms_repeats"]["hip"]]
            ref = [t for r in runs for t in r[f"mask_{size}"][what]["ms_repeats"]["torch"]]
            out[f"mask_{size}_{what}"] = {"hip_ms_range": [min(hip), max(hip)], "torch_ms_range": [min(ref), max(ref)],
                                          "hip_faster_beyond_spread": max(hip) < min(ref)}
    device = [t for r in runs for t in r["running_stats"]["ms_repeats"]["device"]]
    ref = [t for r in runs for t in r["running_stats"]["ms_repeats"]["reference"]]
    out["running_stats"] = {"device_ms_range": [min(device), max(device)], "reference_ms_range": [min(ref), max(ref)],
                            "device_faster_beyond_spread": max(device) < min(ref)}
    out["runs"] = len(runs)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--time-limit", type=int, default=540)
    p.add_argument("--out", default=os.path.join(T.ROOT, "profiles", "spotless_time.json"))
    a = p.parse_args()
    signal.alarm(a.time_limit)
    import gspl_amd  # noqa: F401
    assert torch.cuda.is_available(), "spotless_time measures on the GPU"
    dev = torch.device("cuda:0")
    run = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    for size in MASK_SIZES:
        run[f"mask_{size}"] = measure_mask(size, a, dev)
        torch.cuda.empty_cache()
    run["running_stats"] = measure_stats(a, dev)
    signal.alarm(0)
    result = {"tool": "spotless_time", "runs": []}
    if os.path.exists(a.out):
        with open(a.out) as f:
            previous = json.load(f)
        if previous.get("tool") == "spotless_time":
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

"""One scoring event's arithmetic of the Taming-3DGS density controller BEHIND the renderer: `ops.positive_medians` +
`ops.taming_score_accumulate_` per view (csrc/taming.hip) against the reference's formulation
(internal/density_controllers/taming_3dgs_density_controller.py:455-465, 536-553, restated below word for word: nine `normalize` calls
per view, each an in-place NaN write, a comparison, a boolean-mask gather, a `torch.median`, a divide and a masked scatter, then the
aggregate) in float32 torch ops on the same tensors on the same GPU, in one process, the two routes alternating repeat by repeat.

Workload per N (100 000 and 1 000 000): ten views of nine rows — mean gradients and scale products shared by the views; opacities,
depths, int32 radii, and the four per-pixel sums per view, zero in the ~40 % of the rows a view does not see; the rows are GIVEN (no
rendering is timed).
(a) Whole-event time (ten views), host clock around events that end in a device synchronise, median of `--steps` events per repeat.
(b) Host waits of one event on either side, counted by torch's sync debug mode (`warn`), where it takes effect.
(c) `positive_medians` alone over the nine rows (device events): its three passes read 3 x 36 N bytes; next to it a contiguous read of
    as many bytes as ONE pass (`torch.sum` over 9 N floats) timed in the same run.
(d) The edge map of one 1080p image: `ops.find_edges` on the device against PIL on the host as the reference runs it (`get_edges` +
    the min-max normalisation), and whether the two maps are bit-equal.

Each run of this command APPENDS to `runs` in the output file; `verdict` is computed over every run in it: a route counts as faster
only where its slowest repeat of any run is below the other's fastest.  The process ends itself after `--time-limit` seconds.
  python tools/taming_score_time.py [--steps 5] [--warmup 1] [--repeats 3] [--out profiles/taming_score_time.json]"""
import argparse
import json
import os
import signal
import statistics
import time
import warnings

import _step_time as T  # noqa: F401  (puts the repository root on sys.path)
import torch

VIEWS = 10
SIZES = (100_000, 1_000_000)
COEFFS = dict(grad=25., opac=100., dept=5., radii=10., scale=25., dist=50., loss=10., count=0.1, blend=50.)


def build(N, dev):
    g = torch.Generator().manual_seed(N)
    rnd = lambda: torch.rand(N, generator=g)
    grads = (rnd() * 4e-4 * (rnd() < 0.8)).to(dev)
    scales = torch.exp(torch.randn(N, 3, generator=g) * 0.6 - 4.6).prod(dim=1).to(dev)
    views = []
    for _ in range(VIEWS):
        seen = rnd() < 0.6
        hit = seen & (rnd() < 0.9)
        count = (torch.rand(N, generator=g) * 400).floor() * hit
        views.append(dict(
            visible=seen.to(dev), opac=torch.sigmoid(torch.randn(N, generator=g)).to(dev), dept=((2 + 4 * rnd()) * seen).to(dev),
            radii=((1 + 30 * rnd()).to(torch.int32) * seen).to(dev), dist=(count * rnd() * 5).to(dev), loss=(count * rnd() * 0.3).to(dev),
            count=count.to(dev), blend=(count * rnd() * 0.2).to(dev), w=torch.tensor(50 * (0.02 + 0.1 * float(rnd()[0])), device=dev)))
    return grads, scales, views


def normalize(config_value, value_tensor):
    """`Taming3DGSUtils.normalize`, as written."""
    multiplier = config_value
    value_tensor[value_tensor.isnan()] = 0

    valid_indices = (value_tensor > 0)
    valid_value = value_tensor[valid_indices].to(torch.float32)

    ret_value = torch.zeros_like(value_tensor, dtype=torch.float32)
    ret_value[valid_indices] = multiplier * (valid_value / torch.median(valid_value))

    return ret_value


def torch_event(grads, scales, views):
    importance = torch.zeros_like(grads)
    c = COEFFS
    for v in views:
        g_importance = (normalize(c["grad"], grads) + normalize(c["opac"], v["opac"]) + normalize(c["dept"], v["dept"]) +
                        normalize(c["radii"], v["radii"]) + normalize(c["scale"], scales))
        p_importance = (normalize(c["dist"], v["dist"]) + normalize(c["loss"], v["loss"]) + normalize(c["count"], v["count"]) +
                        normalize(c["blend"], v["blend"]))
        importance += v["w"] * (p_importance + g_importance) * v["visible"]
    return importance


def hip_event(grads, scales, views):
    from gspl_amd import ops
    importance = torch.zeros_like(grads)
    coeffs = list(COEFFS.values())
    for v in views:
        rows = [grads, v["opac"], v["dept"], v["radii"], scales, v["dist"], v["loss"], v["count"], v["blend"]]
        counts, medians = ops.positive_medians(rows)
        ops.taming_score_accumulate_(importance, rows, coeffs, counts, medians, v["w"], v["visible"], n_first=5)
    return importance


def _event_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(samples)


def _alternate(routes, steps, warmup, repeats):
    times = {k: [] for k in routes}
    for rep in range(repeats):
        for k in (list(routes) if rep % 2 == 0 else list(routes)[::-1]):
            times[k].append(_event_ms(routes[k], steps, warmup))
    return {"ms_median_of_repeats": {k: round(statistics.median(v), 4) for k, v in times.items()},
            "ms_repeats": {k: [round(t, 4) for t in v] for k, v in times.items()}}


def host_waits(fn):
    """Synchronising calls of one `fn()` as torch's sync debug mode reports them; None where the mode does not take effect."""
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            torch.ones(1, device="cuda").item()
            if not seen:
                return None
            del seen[:]
            fn()
            return len(seen)
    finally:
        torch.cuda.set_sync_debug_mode(previous)


def _device_ms(fn, inner=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def measure_passes(grads, scales, view, a):
    from gspl_amd import ops
    rows = [grads, view["opac"], view["dept"], view["radii"], scales, view["dist"], view["loss"], view["count"], view["blend"]]
    N = grads.numel()
    flat = torch.rand(9 * N, device=grads.device)
    routes = {"positive_medians": lambda: ops.positive_medians(rows), "contiguous_read_of_one_pass": lambda: torch.sum(flat)}
    times = {k: [] for k in routes}
    for rep in range(a.repeats):
        for k in (list(routes) if rep % 2 == 0 else list(routes)[::-1]):
            for _ in range(a.warmup + 1):
                routes[k]()
            torch.cuda.synchronize()
            times[k].append(statistics.median(_device_ms(routes[k]) for _ in range(a.steps)))
    per_pass = 36 * N
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"bytes_read_per_pass": per_pass, "passes": 3, "ms_repeats": {k: [round(t, 4) for t in v] for k, v in times.items()},
            "GB_per_s_of_the_three_passes": round(3 * per_pass / med["positive_medians"] / 1e6, 1),
            "GB_per_s_of_the_contiguous_read": round(per_pass / med["contiguous_read_of_one_pass"] / 1e6, 1),
            "note": "positive_medians is a memset, three digit passes and three select launches; the read is torch.sum over as many bytes as one pass"}


def measure_edges(dev, a):
    from gspl_amd import ops
    g = torch.Generator().manual_seed(3)
    low = torch.rand(3, 68, 120, generator=g)
    image = torch.nn.functional.interpolate(low[None], size=(1080, 1920), mode="bilinear")[0].clamp(0, 1)
    image = ((image + 0.04 * torch.rand(3, 1080, 1920, generator=g)).clamp(0, 1) * 255).to(torch.uint8)
    on_device = image.to(dev)
    routes = {"hip": lambda: ops.find_edges(on_device)}
    out = {"image": [1080, 1920]}
    try:
        from PIL import Image, ImageFilter
        import numpy as np

        def pil():      # `get_edges` (ToPILImage, convert, filter, ToTensor) and the normalisation of `on_train_start`, on the host
            as_float = image.float() / 255.
            picture = Image.fromarray(as_float.mul(255).byte().permute(1, 2, 0).numpy(), mode="RGB")
            edges = torch.from_numpy(np.array(picture.convert("L").filter(ImageFilter.FIND_EDGES))).to(torch.float32).div(255)
            return (edges - torch.min(edges)) / (torch.max(edges) - torch.min(edges))
        routes["pil_on_the_host"] = pil
        out["bit_equal_to_pil"] = bool(torch.equal(ops.find_edges(on_device).cpu(), pil()))
    except ImportError:
        out["pil_on_the_host"] = "PIL is not installed here"
    out.update(_alternate(routes, a.steps, a.warmup, a.repeats))
    return out


def verdict(runs):
    out = {}
    for case in [k for k in runs[0] if k.startswith("event_")] + ["edges"]:
        hip = [t for r in runs for t in r[case]["ms_repeats"]["hip"]]
        other = "torch" if case != "edges" else "pil_on_the_host"
        ref = [t for r in runs for t in r[case]["ms_repeats"].get(other, [])]
        out[case] = {"hip_ms_range": [min(hip), max(hip)], f"{other}_ms_range": [min(ref), max(ref)] if ref else None,
                     "hip_faster_beyond_spread": bool(ref) and max(hip) < min(ref), "hip_slower_beyond_spread": bool(ref) and min(hip) > max(ref)}
    out["runs"] = len(runs)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--time-limit", type=int, default=420)
    p.add_argument("--out", default=os.path.join(T.ROOT, "profiles", "taming_score_time.json"))
    a = p.parse_args()
    signal.alarm(a.time_limit)
    import gspl_amd  # noqa: F401
    assert torch.cuda.is_available(), "taming_score_time measures on the GPU"
    dev = torch.device("cuda:0")
    run = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "views": VIEWS, "rows": 9}
    for N in SIZES:
        grads, scales, views = build(N, dev)
        routes = {"torch": lambda: torch_event(grads, scales, views), "hip": lambda: hip_event(grads, scales, views)}
        mine, theirs = routes["hip"](), routes["torch"]()
        entry = {"bit_equal_to_the_torch_formulation": bool(torch.equal(mine, theirs)),
                 "max_relative_difference": float(((mine - theirs).abs() / theirs.abs().clamp_min(1e-30)).max())}
        entry["host_waits_per_event"] = {k: host_waits(fn) for k, fn in routes.items()}
        entry.update(_alternate(routes, a.steps, a.warmup, a.repeats))
        entry["positive_medians_alone"] = measure_passes(grads, scales, views[0], a)
        run[f"event_N{N}"] = entry
        del grads, scales, views
    run["edges"] = measure_edges(dev, a)
    signal.alarm(0)
    result = {"tool": "taming_score_time", "runs": []}
    if os.path.exists(a.out):
        with open(a.out) as f:
            previous = json.load(f)
        if previous.get("tool") == "taming_score_time":
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

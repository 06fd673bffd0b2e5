"""What the `*_step_time.py` tools share: the common arguments, a workload with bench.py's heterogeneous 16-camera set on the device,
the loop that alternates the variants round by round inside ONE process (so that clock and thermal drift spread over all of them),
and the medians that go into the JSON line each tool prints."""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def arguments(steps: int, warmup: int, workload=None, variants=None):
    """The parser with --rounds / --steps / --warmup (and --workload, --variants where the tool has them)."""
    p = argparse.ArgumentParser()
    if workload is not None:
        p.add_argument("--workload", default=workload)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=steps)
    p.add_argument("--warmup", type=int, default=warmup)
    if variants is not None:
        p.add_argument("--variants", default=",".join(variants))
    return p


def chosen_variants(a, variants):
    chosen = [v for v in a.variants.split(",") if v]
    assert all(v in variants for v in chosen), chosen
    return chosen


def scene(wl, dev):
    """(means, scales, quats, opacities, shs) of the workload, on the device."""
    from gspl_amd import synthetic
    return [t.to(dev) for t in synthetic.workload_scene(wl, seed=42)]


def load(name: str, dev):
    """The workload `name`: its entry `wl` and size `W`, `H`, the 16 cameras `cams` on the device, the first epoch's camera `order`,
    a zero background `bg`, and a random `target` image with the generator `gen` that drew it."""
    from gspl_amd import synthetic
    wl = synthetic.WORKLOADS[name]
    W, H = wl["width"], wl["height"]
    cams = synthetic.camera_set(W, H, wl["fx"], count=16, distance=wl.get("distance", 4.0))
    cams = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()} for c in cams]
    gen = torch.Generator(device=dev).manual_seed(7)
    return types.SimpleNamespace(wl=wl, W=W, H=H, cams=cams, order=[int(i) for i in synthetic.epoch_order(len(cams), 0)],
                                 bg=torch.zeros(3, device=dev), target=torch.rand(3, H, W, device=dev, generator=gen), gen=gen)


def timed(fn, steps: int, warmup: int, first: int = 0) -> float:
    """Mean device time (ms) of `fn(i)`, i = first .. first + steps - 1, after `warmup` calls that start at `first` as well."""
    for i in range(warmup):
        fn(first + i)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(steps):
        fn(first + i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def alternate(variants, fn, rounds: int, steps: int, warmup: int) -> dict:
    """{variant: [ms per step, one per round]} of `fn(variant, i)`; the variants run in turn, in reverse order every other round, and
    `i` counts the timed steps of the rounds before."""
    times = {v: [] for v in variants}
    for r in range(rounds):
        for v in (variants if r % 2 == 0 else variants[::-1]):
            times[v].append(timed(lambda i: fn(v, i), steps, warmup, first=r * steps))
    return times


def medians(times: dict):
    """(median per variant, the medians rounded for print, every round rounded for print)."""
    med = {v: statistics.median(t) for v, t in times.items()}
    return med, {v: round(m, 4) for v, m in med.items()}, {v: [round(x, 4) for x in t] for v, t in times.items()}


def print_step_times(a, times: dict, extra):
    """The JSON line of a tool whose variants are whole training steps on one workload; `extra(medians)`: the tool's own keys."""
    med, med_print, rounds_print = medians(times)
    print(json.dumps({"workload": a.workload, "cameras": "heterogeneous x16", "rounds": a.rounds, "steps": a.steps,
                      "ms_per_step_median": med_print, "ms_per_step_rounds": rounds_print, **extra(med)}))

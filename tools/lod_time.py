"""The partition-LoD route's per-frame front: `gspl_amd.lod.LoDSelector` (csrc/lod.hip: one select launch, one 16-byte read, one gather
launch when the selection changed) against the reference's formulation (internal/renderers/partition_lod_renderer.py:550-625, restated
below: torch distance and threshold ops, the two `torch.all(torch.eq())` host waits, the Python loop over the partitions with one
`.item()` each, five `torch.concat`), on the same tensors on the same GPU, in one process, the two routes alternating repeat by repeat.

Workload: 256 partitions (16 x 16, side 10) x 3 levels, the finest level 4 000 000 Gaussians in all, each coarser level half of the one
above, SH degree 3 (236 bytes per Gaussian); visibility filter off (the reference's needs pytorch3d).
  `moving`: the camera steps between poses whose selections differ, so EVERY frame gathers.
  `still`:  the same pose every frame: the selection never changes, nothing is gathered.
(a) Whole-call time per frame of the front alone (no rasterization), host clock around frames that end in a device synchronise, median
    of `--steps` frames per repeat.
(b) The gather launch alone over one selection (device events), as bytes read + written per second, next to a contiguous `copy_` of
    the same number of bytes timed in the same run: the ceiling the gather is judged against.

Each run of this command APPENDS to `runs` in the output file; `verdict` is computed over every run in it: a route counts as faster
only where its slowest repeat of any run is below the other's fastest.  The process ends itself after `--time-limit` seconds.
  python tools/lod_time.py [--steps 20] [--warmup 3] [--repeats 3] [--out profiles/lod_time.json]"""
import argparse
import json
import os
import signal
import statistics
import time

import _step_time as T  # noqa: F401  (puts the repository root on sys.path)
import torch

GRID, SIDE, LEVELS, FINEST, K = 16, 10.0, 3, 4_000_000, 16
PROPERTIES = ("means", "shs", "opacities", "scales", "rotations")
BYTES_PER_ROW = 4 * (3 + 3 * K + 1 + 3 + 4)


def build(dev, finest=FINEST):
    """The table, the boxes and the thresholds; partition lengths vary by +-20 % around the mean."""
    from gspl_amd.lod import LoDTable
    P = GRID * GRID
    gen = torch.Generator().manual_seed(5)
    share = 0.8 + 0.4 * torch.rand(P, generator=gen)
    fine = (share / share.sum() * finest).long()
    lengths = [[int(n) >> l for n in fine] for l in range(LEVELS)]
    ij = torch.stack([torch.arange(P) % GRID, torch.arange(P) // GRID], -1).float()
    box_min = ij * SIDE - 0.5 * GRID * SIDE
    box_max = box_min + SIDE

    def segment(n):      # (contents do not matter to a copy; random so that nothing compresses)
        return {"means": torch.rand(n, 3, device=dev), "shs": torch.rand(n, K, 3, device=dev), "opacities": torch.rand(n, 1, device=dev),
                "scales": torch.rand(n, 3, device=dev), "rotations": torch.rand(n, 4, device=dev)}
    table = LoDTable([[segment(n) for n in level] for level in lengths], device=dev)
    thresholds = torch.tensor([2.0 * SIDE, 5.0 * SIDE])
    return table, box_min.to(dev), box_max.to(dev), thresholds.to(dev)


class TorchFront:
    """The reference's per-frame formulation in this tool's words, over per-partition slices of the same table: torch ops for the
    distances and one masked assignment per threshold, the two `torch.all(torch.eq())` host reads that compare the choice with the
    stored one, and on a change one `.item()` per partition and one `torch.concat` per property."""

    def __init__(self, table, box_min, box_max, thresholds):
        P, starts = table.n_partitions, table.seg_start.tolist()
        cut = lambda l, p: slice(starts[l * P + p], starts[l * P + p + 1])
        self.segments = [[[table.arrays[k][cut(l, p)] for k in PROPERTIES] for p in range(P)] for l in range(table.n_levels)]
        self.lo, self.hi, self.limits = box_min, box_max, thresholds
        self.to_grid = torch.eye(3, device=box_min.device)
        self.stored_levels = torch.full((P,), 127, dtype=torch.int8, device=box_min.device)
        self.stored_shown = torch.ones(P, dtype=torch.bool, device=box_min.device)
        self.gathered, self.n_updates = [], 0

    def distances(self, centre):
        xy = (centre @ self.to_grid)[:2]
        outside = torch.maximum(self.lo - xy, xy - self.hi).clamp(min=0.)
        return torch.sqrt(torch.pow(outside, 2).sum(dim=-1))

    def frame(self, centre):
        far = self.distances(centre)
        levels = torch.full_like(self.stored_levels, -1)          # -1 indexes the coarsest level
        for i in reversed(range(len(self.segments) - 1)):
            levels[far < self.limits[i]] = i
        shown = torch.ones_like(self.stored_shown)                # filter off
        same = torch.all(torch.eq(self.stored_levels, levels)) and torch.all(torch.eq(self.stored_shown, shown))      # two host reads
        if not same:
            self.stored_levels, self.stored_shown = levels, shown
            columns = [[] for _ in PROPERTIES]
            for p, level in enumerate(levels):
                if shown[p]:                                      # (a host read per partition, as the reference has it)
                    for column, rows in zip(columns, self.segments[level.item()][p]):
                        column.append(rows)
            self.gathered = [torch.concat(column, dim=0) for column in columns]
            self.n_updates += 1
        return dict(zip(PROPERTIES, self.gathered))


def poses(dev):
    """Camera centres over the grid: `moving` steps by 1.7 partition sides per frame along a diagonal and back, so that consecutive
    frames always differ in some partition's level; `still` is its first pose."""
    xs = [(-0.4 * GRID + 1.7 * i) * SIDE for i in range(8)]
    path = xs + xs[-2:0:-1]
    return [torch.tensor([x, 0.6 * x + 3.0, 25.0], device=dev) for x in path]


def _frame_ms(fn, centres, steps, warmup):
    for i in range(warmup):
        fn(centres[i % len(centres)])
    torch.cuda.synchronize()
    samples = []
    for i in range(steps):
        t0 = time.perf_counter()
        fn(centres[(warmup + i) % len(centres)])
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(samples)


def _alternate(routes, centres, steps, warmup, repeats):
    times = {k: [] for k in routes}
    for rep in range(repeats):
        for k in (list(routes) if rep % 2 == 0 else list(routes)[::-1]):
            times[k].append(_frame_ms(routes[k], centres, steps, warmup))
    return times


def _summary(times):
    return {"ms_median_of_repeats": {k: round(statistics.median(v), 4) for k, v in times.items()},
            "ms_repeats": {k: [round(t, 4) for t in v] for k, v in times.items()}}


def _event_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def measure_gather(table, selector, a):
    """The gather launch alone on the selector's current selection against one contiguous copy_ of as many bytes."""
    from gspl_amd import ops
    n = selector.n_gaussians
    out = table.reserve(n)
    floats = n * BYTES_PER_ROW // 4
    src, dst = torch.rand(floats, device=table.device), torch.empty(floats, device=table.device)
    routes = {"gather": lambda: ops.lod_gather(table.seg_start, selector.lod, selector.dst_start, n, *[table.arrays[k] for k in PROPERTIES], out=out),
              "copy_": lambda: dst.copy_(src)}
    times = {k: [] for k in routes}
    for rep in range(a.repeats):
        for k in (list(routes) if rep % 2 == 0 else list(routes)[::-1]):
            for _ in range(a.warmup):
                routes[k]()
            torch.cuda.synchronize()
            times[k].append(statistics.median(_event_ms(routes[k], 10) for _ in range(a.steps)))
    moved = 2 * n * BYTES_PER_ROW
    return {"rows": n, "bytes_read_and_written": moved, **_summary(times),
            "GB_per_s_median": {k: round(moved / statistics.median(v) / 1e6, 1) for k, v in times.items()},
            "GB_per_s_repeats": {k: [round(moved / t / 1e6, 1) for t in v] for k, v in times.items()}}


def verdict(runs):
    out = {}
    for case in ("moving", "still"):
        hip = [t for r in runs for t in r[case]["ms_repeats"]["hip"]]
        ref = [t for r in runs for t in r[case]["ms_repeats"]["torch"]]
        out[case] = {"hip_ms_range": [min(hip), max(hip)], "torch_ms_range": [min(ref), max(ref)], "hip_faster_beyond_spread": max(hip) < min(ref)}
    gather = [t for r in runs for t in r["gather"]["ms_repeats"]["gather"]]
    copy = [t for r in runs for t in r["gather"]["ms_repeats"]["copy_"]]
    out["gather_vs_copy"] = {"gather_ms_range": [min(gather), max(gather)], "copy_ms_range": [min(copy), max(copy)],
                             "gather_slower_beyond_spread": min(gather) > max(copy), "gather_over_copy_medians": round(statistics.median(gather) / statistics.median(copy), 3)}
    out["runs"] = len(runs)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--finest", type=int, default=FINEST)
    p.add_argument("--time-limit", type=int, default=420)
    p.add_argument("--out", default=os.path.join(T.ROOT, "profiles", "lod_time.json"))
    a = p.parse_args()
    signal.alarm(a.time_limit)
    import gspl_amd  # noqa: F401
    from gspl_amd.lod import LoDSelector
    assert torch.cuda.is_available(), "lod_time measures on the GPU"
    dev = torch.device("cuda:0")
    table, box_min, box_max, thresholds = build(dev, a.finest)
    selector = LoDSelector(table, box_min, box_max, thresholds)
    front = TorchFront(table, box_min, box_max, thresholds)
    centres = poses(dev)

    # the two routes choose and gather the same rows, on every pose of the path
    selections, rows = set(), []
    for c in centres:
        selector.select(c)
        mine, theirs = table.views(), front.frame(c)
        assert all(torch.equal(mine[k], theirs[k]) for k in PROPERTIES)
        selections.add(tuple(selector.lod.tolist()))
        assert selector.lod.tolist() == [l % LEVELS for l in front.stored_levels.tolist()]
        rows.append(selector.n_gaussians)
    gathers, updates = selector.n_gathers, front.n_updates
    run = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "partitions": GRID * GRID, "levels": LEVELS,
           "table_rows": table.n_rows, "finest_level_rows": sum(table.segment_lengths[:GRID * GRID]), "bytes_per_row": BYTES_PER_ROW,
           "distinct_selections_on_the_path": len(selections), "rows_selected_on_the_path": [min(rows), max(rows)]}
    routes = {"torch": front.frame, "hip": lambda c: selector.select(c)}
    run["moving"] = _summary(_alternate(routes, centres, a.steps, a.warmup, a.repeats))
    frames = a.repeats * (a.steps + a.warmup)
    run["moving"]["frames"], run["moving"]["frames_that_gathered"] = frames, {"hip": selector.n_gathers - gathers, "torch": front.n_updates - updates}
    # (the first frame of a repeat may meet the pose the repeat before it ended on)
    assert min(run["moving"]["frames_that_gathered"].values()) >= frames - a.repeats, "frames of the moving path did not change the selection"
    gathers, updates = selector.n_gathers, front.n_updates
    run["still"] = _summary(_alternate(routes, centres[:1], a.steps, a.warmup, a.repeats))
    assert selector.n_gathers - gathers <= 1 and front.n_updates - updates <= 1
    run["gather"] = measure_gather(table, selector, a)
    signal.alarm(0)
    result = {"tool": "lod_time", "runs": []}
    if os.path.exists(a.out):
        with open(a.out) as f:
            previous = json.load(f)
        if previous.get("tool") == "lod_time":
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

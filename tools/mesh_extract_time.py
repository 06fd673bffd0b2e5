"""TSDF fusion of one lattice block: `ops.tsdf_fuse` (one launch for all views, the lattice never materialised) against the reference's
formulation restated with torch ops (tests/mesh_oracle.py `fuse_torch`: per view a matrix product, a division, a `grid_sample` and
masked scatter updates), float32, on the same GPU, in one process, the two routes alternating repeat by repeat.

The comparison favours the torch route: its [M, 3] point tensor is built before the clock starts and the maps are on the device already
(the reference copies every map from the CPU for every chunk and camera), and it fuses depth only, as the kernel does here.

Workload: a 256^3 lattice in contracted space over [-1.2, 1.2]^3, 16 views of 400 x 400 of the analytic sphere scene of the tests.
Per repeat the MEDIAN of `--steps` runs, each between its own pair of device events.  Also timed, kernel route only: marching
tetrahedra (count, prefix sum, emit, merge by key) on the fused volume.  Writes one JSON object to --out and prints it.

Traffic model of the fusion kernel: the state is read and written once per call (tsdf and weight: 16 bytes per sample) and every map is
fetched from memory once (4 V H W bytes; the taps of neighbouring samples hit the caches): the bytes that MUST move.  `fraction_of_8TBs`
is that figure over the median time over 8e12 B/s.
  python tools/mesh_extract_time.py [--n 256] [--views 16] [--size 400] [--steps 5] [--warmup 2] [--repeats 3] [--out profiles/mesh_extract_time.json]"""
import argparse
import json
import os
import statistics
import sys

import _step_time as T  # noqa: F401  (puts the repository root on sys.path)
import torch

sys.path.insert(0, os.path.join(T.ROOT, "tests"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=256)
    p.add_argument("--views", type=int, default=16)
    p.add_argument("--size", type=int, default=400)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=os.path.join(T.ROOT, "profiles", "mesh_extract_time.json"))
    a = p.parse_args()
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    import mesh_oracle as MO
    assert torch.cuda.is_available(), "mesh_extract_time measures on the GPU"
    dev = torch.device("cuda:0")
    n, V, S = a.n, a.views, a.size
    M = n ** 3
    full, _, geo = MO.orbit_cameras(V, S, S)
    depth_np, _ = MO.sphere_maps(geo, S, S)
    views, depth = torch.from_numpy(full).to(dev), torch.from_numpy(depth_np).to(dev)
    center, radius, voxel = torch.tensor([0.03, -0.02, 0.01], device=dev), 1.0, 2.0 / n
    lo, hi = (-1.2,) * 3, (1.2,) * 3
    table = ops.tsdf_table(center, radius, voxel, contract=True, lo=lo, hi=hi, device=dev)
    axis = torch.tensor(lo[0], device=dev) + torch.arange(n, device=dev, dtype=torch.float32) * ((torch.tensor(hi[0], device=dev) - lo[0]) / (n - 1))
    points = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()

    def kernel():
        state = ops.tsdf_init(M, False, dev)
        ops.tsdf_fuse(state, table, views, depth, lattice=(n, n, n))
        return state

    def restated():
        return MO.fuse_torch(points, views, depth, None, center=center, radius=radius, voxel_size=voxel, contract=True)

    # the two routes fuse the same volume at the size that is timed
    k, r = kernel(), restated()
    same_weight = float((k[1] == r[1]).float().mean())
    agree = k[1] == r[1]
    worst = float((k[0] - r[0]).abs()[agree].max())
    fused = float((k[1] > 1).float().mean())
    volume = k[0].view(n, n, n).clone()
    del k, r
    routes = {"restated": restated, "kernel": kernel}
    medians = {name: [] for name in routes}
    for rep in range(a.repeats):
        for name in (list(routes) if rep % 2 == 0 else list(routes)[::-1]):
            for _ in range(a.warmup):
                routes[name]()
            torch.cuda.synchronize()
            events = []
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                routes[name]()
                e1.record()
                events.append((e0, e1))
            torch.cuda.synchronize()
            medians[name].append(statistics.median(e0.elapsed_time(e1) for e0, e1 in events))
    # the kernel alone, without the state's initialisation (two fills)
    state = ops.tsdf_init(M, False, dev)
    alone = []
    for _ in range(a.warmup + a.steps * a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.tsdf_fuse(state, table, views, depth, lattice=(n, n, n))
        e1.record()
        alone.append((e0, e1))
    torch.cuda.synchronize()
    alone_ms = statistics.median(e0.elapsed_time(e1) for e0, e1 in alone[a.warmup:])
    del state
    step = [(h - l) / (n - 1) for l, h in zip(lo, hi)]
    mt = []
    for _ in range(a.warmup + a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        mesh = ops.marching_tetrahedra(volume, 0.0, lo, step)
        e1.record()
        mt.append((e0, e1))
    torch.cuda.synchronize()
    mt_ms = statistics.median(e0.elapsed_time(e1) for e0, e1 in mt[a.warmup:])
    bytes_moved = 16 * M + 4 * V * S * S
    med = {k: statistics.median(v) for k, v in medians.items()}
    result = {
        "tool": "mesh_extract_time", "lattice": [n, n, n], "views": V, "image": [S, S], "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
        "device": torch.cuda.get_device_name(0),
        "ms_median_of_repeats": {k: round(v, 4) for k, v in med.items()},
        "ms_repeats": {k: [round(x, 4) for x in v] for k, v in medians.items()},
        "speedup": round(med["restated"] / med["kernel"], 2),
        "kernel_faster_beyond_spread": max(medians["kernel"]) < min(medians["restated"]),
        "fuse_kernel_alone_ms": round(alone_ms, 4), "fuse_kernel_bytes": bytes_moved,
        "fuse_kernel_GBs": round(bytes_moved / (alone_ms * 1e-3) / 1e9, 1), "fraction_of_8TBs": round(bytes_moved / (alone_ms * 1e-3) / 8e12, 4),
        "samples_with_a_fused_view": round(fused, 4), "share_of_samples_with_equal_weight": same_weight, "worst_tsdf_difference_where_equal": worst,
        "marching_tetrahedra_ms": round(mt_ms, 4), "triangles": int(mesh[1].shape[0]), "vertices": int(mesh[0].shape[0]),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

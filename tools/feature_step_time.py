"""Forward + backward of a wide feature map over a frozen model, the route that existed before `ops.rasterize_features` against that
op.  One process, the two paths alternating repeat by repeat so that clock and thermal drift spread over both.

  batched   `HipGSplatRenderer.rasterize_simplified` in batches of 32 channels with `features.requires_grad` — what the reference's
            Feature3DGSRenderer loop runs on the `gsplat` stand-in: per batch one binning, the channel adapter's four 8-channel
            forwards and four general backwards
  features  one `ops.rasterize_features` call (one binning, csrc/features.hip)

Workload: S-800-100k (100 000 Gaussians at 800x800), the projection done once outside the timed region (Feature-3DGS projects under
no_grad, identically on both paths), D = 128 and 256, the loss a fixed random weighting of the map.  Per repeat the MEDIAN of
`--steps` steps, each timed with its own pair of device events; `--repeats` repeats per path.  The verdict per width: the op is
faster when its slowest repeat beats the batched route's fastest, i.e. by more than the spread of the repeats.  Prints one JSON line.
  python tools/feature_step_time.py [--dims 128,256] [--steps 50] [--warmup 5] [--repeats 3]"""
import argparse
import json
import statistics

import _step_time as T  # noqa: F401  (puts the repository root on sys.path)
import torch


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--workload", default="S-800-100k")
    p.add_argument("--dims", default="128,256")
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=3)
    a = p.parse_args()
    import gspl_amd  # noqa: F401
    from gspl_amd import ops, synthetic
    from gspl_amd.renderers import HipGSplatRenderer
    assert torch.cuda.is_available(), "feature_step_time measures on the GPU"
    assert a.steps >= 1 and a.repeats >= 1
    dev = torch.device("cuda:0")
    wl = synthetic.WORKLOADS[a.workload]
    W, H = wl["width"], wl["height"]
    means, scales, quats, opac, _ = T.scene(wl, dev)
    cam = synthetic.camera(W, H, wl["fx"])

    class Camera:
        world_to_camera = cam["world_to_camera"].to(dev)
        fx, fy, cx, cy = (torch.tensor(float(cam[k]), device=dev) for k in ("fx", "fy", "cx", "cy"))
        width, height = torch.tensor(W, device=dev), torch.tensor(H, device=dev)
    camera = Camera()
    with torch.no_grad():
        proj = HipGSplatRenderer.project(means, scales, quats, camera)
        xys, depths, radii, conics, comp, tiles, _ = proj
        opacities = opac * comp[:, None]
    gen = torch.Generator(device=dev).manual_seed(7)
    result = {"tool": "feature_step_time", "workload": a.workload, "n": wl["n"], "width": W, "height": H, "steps": a.steps,
              "warmup": a.warmup, "repeats": a.repeats}

    for D in [int(d) for d in a.dims.split(",") if d]:
        features = torch.randn(wl["n"], D, device=dev, generator=gen).requires_grad_(True)
        weight = torch.randn(D, H, W, device=dev, generator=gen)
        zero = torch.zeros(32, device=dev)

        def batched():
            maps = [HipGSplatRenderer.rasterize_simplified(proj, camera, features[:, s:s + 32], zero[:min(32, D - s)], opacities, anti_aliased=False)
                    for s in range(0, D, 32)]
            return torch.cat(maps, dim=0)

        def fused():
            return ops.rasterize_features(xys, depths, radii, conics, tiles, features, opacities, H, W, 16, channels_first=True)

        paths = {"batched": batched, "features": fused}

        def step(fn):
            features.grad = None
            (fn() * weight).sum().backward()

        # the two paths compute the same map (bit for bit) and the same gradient (atomics: to rounding) at the size that is timed
        step(batched)
        g_batched, m_batched = features.grad.clone(), batched().detach()
        step(fused)
        same_map = bool(torch.equal(fused().detach(), m_batched))
        scale = g_batched.abs() + g_batched.square().mean().sqrt()
        grad_diff = float(((features.grad - g_batched).abs() / scale).max())
        del m_batched

        medians = {name: [] for name in paths}
        for r in range(a.repeats):
            for name in (list(paths) if r % 2 == 0 else list(paths)[::-1]):
                for _ in range(a.warmup):
                    step(paths[name])
                torch.cuda.synchronize()
                events = []
                for _ in range(a.steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    step(paths[name])
                    e1.record()
                    events.append((e0, e1))
                torch.cuda.synchronize()
                medians[name].append(statistics.median(e0.elapsed_time(e1) for e0, e1 in events))
        result[f"D{D}"] = {
            "ms_per_step_median_of_repeats": {k: round(statistics.median(v), 4) for k, v in medians.items()},
            "ms_per_step_repeats": {k: [round(x, 4) for x in v] for k, v in medians.items()},
            "speedup": round(statistics.median(medians["batched"]) / statistics.median(medians["features"]), 3),
            "features_faster_beyond_spread": max(medians["features"]) < min(medians["batched"]),
            "same_map_bitwise": same_map, "worst_gradient_difference_rel": grad_diff,
        }
        del features, weight
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()

"""Step time of the fused Inria call with the Taming-3DGS switches, on bench.py's metric workload (S-1080p-1M, the heterogeneous
16-camera set, one camera per step, a fresh permutation per epoch).  Variants, alternated round by round inside ONE process so that
clock and thermal drift spread over all of them:

  default     GaussianRasterizer (raw parameters, shs / shs_rest) + FusedAdam — the bench's vanilla step without its loss kernel
  aa          the same through rasterize_inria_accel(antialiasing=True)
  aa_invd     ... and inverse_depth=True, an L1 term on the inverse depth in the loss
  aa_sparse   aa with SparseGaussianAdam (visibility = radii > 0) instead of FusedAdam

Prints one JSON line: per variant the median over rounds of the mean step time (ms) and its ratio to `default`.
  python tools/accel_step_time.py [--workload S-1080p-1M] [--rounds 5] [--steps 40] [--warmup 10] [--variants a,b,...]
Under `rocprofv3 --kernel-trace --stats -- python tools/accel_step_time.py --variants aa_invd --rounds 1` it gives per-kernel
figures of one variant."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

VARIANTS = ("default", "aa", "aa_invd", "aa_sparse")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--workload", default="S-1080p-1M")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--variants", default=",".join(VARIANTS))
    a = p.parse_args()
    import gspl_amd  # noqa: F401
    from gspl_amd import ops, optimizers, synthetic
    variants = [v for v in a.variants.split(",") if v]
    assert all(v in VARIANTS for v in variants), variants
    dev = torch.device("cuda:0")
    wl = synthetic.WORKLOADS[a.workload]
    W, H = wl["width"], wl["height"]
    means, scales, quats, opac, shs = [t.to(dev) for t in synthetic.workload_scene(wl, seed=42)]
    cams = synthetic.camera_set(W, H, wl["fx"], count=16, distance=wl.get("distance", 4.0))
    cams = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()} for c in cams]
    bg = torch.zeros(3, device=dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    target = torch.rand(3, H, W, device=dev, generator=gen)
    target_inv = torch.rand(1, H, W, device=dev, generator=gen) * 0.3
    raw = [torch.nn.Parameter(t.clone()) for t in (means, scales.log(), quats, torch.logit(opac.clamp(1e-4, 1 - 1e-4)),
                                                   shs[:, :1].contiguous(), shs[:, 1:].contiguous())]

    def make(variant):
        params = [torch.nn.Parameter(t.detach().clone()) for t in raw]
        groups = [{"params": [q], "name": n} for q, n in zip(params, ("xyz", "scaling", "rotation", "opacity", "f_dc", "f_rest"))]
        opt = optimizers.SparseGaussianAdam(groups, lr=1e-4, eps=1e-15) if variant == "aa_sparse" else optimizers.FusedAdam(groups, lr=1e-4)
        return params, opt

    def step(variant, params, opt, cam):
        m, s, q, o, dc, rest = params
        st = ops.AccelRasterizationSettings(H, W, cam["tanfovx"], cam["tanfovy"], bg, 1.0, cam["world_to_camera"], cam["full_projection"], 3,
                                            cam["camera_center"], antialiasing=variant != "default")
        screen = torch.empty_like(m).requires_grad_(True)
        if variant == "default":
            img, radii = ops.GaussianRasterizer(ops.GaussianRasterizationSettings(*st[:-1]))(m, screen, o, shs=dc, shs_rest=rest, scales=s, rotations=q,
                                                                                             raw_parameters=True)
            inv = None
        else:
            img, radii, inv = ops.rasterize_inria_accel(st, m, screen, o, dc, scales=s, rotations=q, shs_rest=rest, raw_parameters=True,
                                                        antialiasing=True, inverse_depth=variant == "aa_invd")
        loss = (img - target).abs().mean()
        if inv is not None:
            loss = loss + 0.1 * (inv - target_inv).abs().mean()
        loss.backward()
        if variant == "aa_sparse":
            opt.step(radii > 0, radii.shape[0])
        else:
            opt.step()
        opt.zero_grad(set_to_none=True)

    state = {v: make(v) for v in variants}
    order = [int(i) for i in synthetic.epoch_order(len(cams), 0)]
    times = {v: [] for v in variants}
    k = 0
    for r in range(a.rounds):
        for v in (variants if r % 2 == 0 else variants[::-1]):
            params, opt = state[v]
            for i in range(a.warmup):
                step(v, params, opt, cams[order[(k + i) % len(order)]])
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(a.steps):
                step(v, params, opt, cams[order[(k + i) % len(order)]])
            t1.record()
            torch.cuda.synchronize()
            times[v].append(t0.elapsed_time(t1) / a.steps)
        k += a.steps
    med = {v: statistics.median(times[v]) for v in variants}
    base = med.get("default")
    print(json.dumps({"workload": a.workload, "cameras": "heterogeneous x16", "rounds": a.rounds, "steps": a.steps,
                      "ms_per_step_median": {v: round(med[v], 4) for v in variants},
                      "ms_per_step_rounds": {v: [round(x, 4) for x in times[v]] for v in variants},
                      "ratio_to_default": ({v: round(med[v] / base, 4) for v in variants} if base else None),
                      "speculation": dict(ops.SPECULATION)}))


if __name__ == "__main__":
    main()

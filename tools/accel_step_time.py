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
import torch

import _step_time as T

VARIANTS = ("default", "aa", "aa_invd", "aa_sparse")


def main():
    a = T.arguments(steps=40, warmup=10, workload="S-1080p-1M", variants=VARIANTS).parse_args()
    import gspl_amd  # noqa: F401
    from gspl_amd import ops, optimizers
    variants = T.chosen_variants(a, VARIANTS)
    dev = torch.device("cuda:0")
    w = T.load(a.workload, dev)
    W, H, cams, order, bg, target = w.W, w.H, w.cams, w.order, w.bg, w.target
    means, scales, quats, opac, shs = T.scene(w.wl, dev)
    target_inv = torch.rand(1, H, W, device=dev, generator=w.gen) * 0.3
    raw = [torch.nn.Parameter(t.clone()) for t in (means, scales.log(), quats, torch.logit(opac.clamp(1e-4, 1 - 1e-4)),
                                                   shs[:, :1].contiguous(), shs[:, 1:].contiguous())]

    def make(variant):
        params = [torch.nn.Parameter(t.detach().clone()) for t in raw]
        groups = [{"params": [q], "name": n} for q, n in zip(params, ("xyz", "scaling", "rotation", "opacity", "f_dc", "f_rest"))]
        opt = optimizers.SparseGaussianAdam(groups, lr=1e-4, eps=1e-15) if variant == "aa_sparse" else optimizers.FusedAdam(groups, lr=1e-4)
        return params, opt

    def step(variant, i):
        (m, s, q, o, dc, rest), opt = state[variant]
        cam = cams[order[i % len(order)]]
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
    times = T.alternate(variants, step, a.rounds, a.steps, a.warmup)
    T.print_step_times(a, times, lambda med: {
        "ratio_to_default": ({v: round(med[v] / med["default"], 4) for v in variants} if med.get("default") else None),
        "speculation": dict(ops.SPECULATION)})


if __name__ == "__main__":
    main()

"""Step time of the 2DGS (surfel) rasterizer against the fused Inria step, on bench.py's metric workload (S-1080p-1M, the heterogeneous
16-camera set, one camera per step).  Variants, alternated round by round inside ONE process so that clock and thermal drift spread over
both:

  vanilla   GaussianRasterizer (raw parameters, shs / shs_rest) + FusedAdam, the L1 + SSIM loss
  surfel    HipVanilla2DGSRenderer forward, the L1 + SSIM loss plus GS2D's normal-consistency and distortion terms, backward, and Adam
            (FusedAdam over the activated parameters: the 2DGS renderer takes the model's activated values)
  surfel-fused  the same step with `HipVanilla2DGSRenderer(fused_maps=True)` (everything after the rasterizer is `ops.surfel_maps`) and
            the two regularisers from one `ops.surface_reg` call (csrc/normals.hip)

Prints one JSON line: per variant the median over rounds of the mean step time (ms), the surfel / vanilla and the surfel-fused / surfel
ratios where both were run.
  python tools/surfel_step_time.py [--workload S-1080p-1M] [--rounds 5] [--steps 30] [--warmup 8] [--variants vanilla,surfel]
Under `rocprofv3 --kernel-trace --stats -- python tools/surfel_step_time.py --variants surfel --rounds 1` it gives per-kernel figures."""
import torch

import _step_time as T

VARIANTS = ("vanilla", "surfel", "surfel-fused")


class _Camera:
    """The fields of the reference's Camera the renderers read (internal/cameras/cameras.py)."""

    def __init__(self, cam, dev):
        import math
        self.world_to_camera, self.full_projection, self.camera_center = cam["world_to_camera"], cam["full_projection"], cam["camera_center"]
        self.width = torch.tensor(cam["width"], dtype=torch.int32, device=dev)
        self.height = torch.tensor(cam["height"], dtype=torch.int32, device=dev)
        self.fov_x = torch.tensor(2 * math.atan(cam["tanfovx"]), device=dev)
        self.fov_y = torch.tensor(2 * math.atan(cam["tanfovy"]), device=dev)


class _SurfelModel:
    """Activated 2DGS parameters in the getters `Vanilla2DGSRenderer` reads (internal/models/gaussian_2d.py)."""

    def __init__(self, params):
        self.params = params
        self.active_sh_degree = 3

    get_xyz = property(lambda s: s.params[0])
    get_scaling = property(lambda s: s.params[1])
    get_rotation = property(lambda s: s.params[2])
    get_opacity = property(lambda s: s.params[3])
    get_features = property(lambda s: s.params[4])


def main():
    a = T.arguments(steps=30, warmup=8, workload="S-1080p-1M", variants=VARIANTS[:2]).parse_args()
    import gspl_amd  # noqa: F401
    from gspl_amd import ops, optimizers
    from gspl_amd.renderers import HipVanilla2DGSRenderer
    variants = T.chosen_variants(a, VARIANTS)
    dev = torch.device("cuda:0")
    w = T.load(a.workload, dev)
    W, H, cams, order, bg, target = w.W, w.H, w.cams, w.order, w.bg, w.target
    means, scales, quats, opac, shs = T.scene(w.wl, dev)
    rcams = [_Camera(c, dev) for c in cams]
    renderer = HipVanilla2DGSRenderer(depth_ratio=0.0)
    fused_renderer = HipVanilla2DGSRenderer(depth_ratio=0.0, fused_maps=True)

    def make(variant):
        if variant == "vanilla":
            params = [torch.nn.Parameter(t.clone()) for t in (means, scales.log(), quats, torch.logit(opac.clamp(1e-4, 1 - 1e-4)),
                                                             shs[:, :1].contiguous(), shs[:, 1:].contiguous())]
        else:
            params = [torch.nn.Parameter(t.clone()) for t in (means, scales, quats, opac, shs)]
        groups = [{"params": [q], "name": str(i)} for i, q in enumerate(params)]
        return params, optimizers.FusedAdam(groups, lr=1e-4)

    def step(variant, i):
        params, opt = state[variant]
        ci = order[i % len(order)]
        cam = cams[ci]
        if variant == "vanilla":
            m, s, q, o, dc, rest = params
            st = ops.GaussianRasterizationSettings(H, W, cam["tanfovx"], cam["tanfovy"], bg, 1.0, cam["world_to_camera"], cam["full_projection"], 3,
                                                   cam["camera_center"])
            screen = torch.empty_like(m).requires_grad_(True)
            img, _ = ops.GaussianRasterizer(st)(m, screen, o, shs=dc, shs_rest=rest, scales=s, rotations=q, raw_parameters=True)
            l1, ssim = ops.l1_ssim(img, target)
            loss = 0.8 * l1 + 0.2 * (1 - ssim)
        elif variant == "surfel-fused":
            out = fused_renderer(rcams[ci], _SurfelModel(params), bg)
            l1, ssim = ops.l1_ssim(out["render"], target)
            reg = ops.surface_reg(out["rend_normal"], out["surf_normal"], out["rend_dist"])
            loss = 0.8 * l1 + 0.2 * (1 - ssim) + 0.05 * reg[0] + 100.0 * reg[1]
        else:
            out = renderer(rcams[ci], _SurfelModel(params), bg)
            l1, ssim = ops.l1_ssim(out["render"], target)
            normal_error = (1 - (out["rend_normal"] * out["surf_normal"]).sum(dim=0))[None]
            loss = 0.8 * l1 + 0.2 * (1 - ssim) + 0.05 * normal_error.mean() + 100.0 * out["rend_dist"].mean()
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)

    state = {v: make(v) for v in variants}
    times = T.alternate(variants, step, a.rounds, a.steps, a.warmup)
    ratio = lambda med, x, y: round(med[x] / med[y], 4) if x in med and y in med else None
    T.print_step_times(a, times, lambda med: {"ratio_surfel_to_vanilla": ratio(med, "surfel", "vanilla"),
                                              "ratio_fused_to_surfel": ratio(med, "surfel-fused", "surfel")})


if __name__ == "__main__":
    main()

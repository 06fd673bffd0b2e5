"""Cost of the bilateral-grid route's per-step work, a torch formulation against this package's HIP ops.  Variants alternate round by
round inside ONE process so that clock and thermal drift spread over both.

The torch formulation is written here from the semantics of include/gspl_hip.h section 14 in the shape of the formulation the
`fused_bilagrid` package replaces: `torch.unique` of the index (a host synchronisation), the selected grids gathered, `grid_sample`
(bilinear, align_corners, border) on (2x - 1, 2y - 1, 2 gray - 1), the 3x4 affine as a matmul; TV as three index_select / sub / pow /
sum chains.

  (i)   slice forward + backward at 1080p (one image, grid 16 x 16 x 8, N = 300 grids), the image a channels-last view of a CHW render;
  (ii)  TV forward + backward at N = 2, 300, 2000;
  (iii) the S-1080p-1M training step (GaussianRasterizer on the raw parameters, L1 + SSIM, backward, FusedAdam; bench's default
        configuration) without the processor, and with it: slice + 10 TV + torch Adam (lr 2e-3, eps 1e-15) over the N = 300 grids.

Prints one JSON line.  `--slice-only K` runs K slice forward + backward pairs at 1080p and a TV forward + backward at N = 300, and
nothing else (for `rocprofv3 --kernel-trace --stats`).
  python tools/bilagrid_step_time.py [--rounds 5] [--steps 20] [--warmup 5]"""
import json

import torch
import torch.nn.functional as F

import _step_time as T

GRAY = (0.299, 0.587, 0.114)
N_GRIDS = 300


def torch_slice(grids, xy, rgb, grid_idx):
    B = rgb.shape[0]
    uniq = torch.unique(grid_idx)
    idx = uniq if len(uniq) == 1 else grid_idx.reshape(B, -1)[:, 0]
    sel = grids[idx]
    gray = rgb @ torch.tensor([GRAY], device=rgb.device, dtype=rgb.dtype).T
    coords = torch.cat([(xy.expand(B, *xy.shape[1:]) - 0.5) * 2, gray * 2 - 1], dim=-1).unsqueeze(1)
    if sel.shape[0] != B:
        sel = sel.expand(B, *sel.shape[1:])
    A = F.grid_sample(sel, coords, mode="bilinear", align_corners=True, padding_mode="border")       # [B, 12, 1, H, W]
    A = A.squeeze(2).permute(0, 2, 3, 1).reshape(*rgb.shape[:-1], 3, 4)
    return torch.matmul(A[..., :3], rgb.unsqueeze(-1)).squeeze(-1) + A[..., 3]


def torch_tv(x):
    tv = 0
    for i in range(2, x.dim()):
        n = x.shape[i]
        x1 = x.index_select(i, torch.arange(1, n, device=x.device))
        x2 = x.index_select(i, torch.arange(0, n - 1, device=x.device))
        tv = tv + torch.pow(x1 - x2, 2).sum() / max(x1[0].numel(), 1)
    return tv / x.shape[0]


def hip_slice(grids, xy, rgb, grid_idx):
    from gspl_amd import ops
    return ops.bilagrid_slice(grids, xy, rgb, grid_idx)


def hip_tv(x):
    from gspl_amd import ops
    return ops.bilagrid_tv(x)


SLICE = {"torch": torch_slice, "hip": hip_slice}
TV = {"torch": torch_tv, "hip": hip_tv}


def _alternate(fn, rounds, steps, warmup):
    med, med_print, rounds_print = T.medians(T.alternate(("torch", "hip"), lambda v, _i: fn(v), rounds, steps, warmup))
    return {"ms_median": med_print, "ms_rounds": rounds_print, "speedup": round(med["torch"] / med["hip"], 2)}


def _grids(n, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    ident = torch.tensor([1., 0, 0, 0, 0, 1., 0, 0, 0, 0, 1., 0], device=dev).reshape(1, 12, 1, 1, 1)
    return (ident + 0.05 * torch.randn(n, 12, 8, 16, 16, device=dev, generator=g)).contiguous()


def main():
    p = T.arguments(steps=20, warmup=5, workload="S-1080p-1M")
    p.add_argument("--slice-only", type=int, default=0)
    a = p.parse_args()
    import gspl_amd  # noqa: F401
    assert torch.cuda.is_available(), "bilagrid_step_time measures on the GPU"
    dev = torch.device("cuda:0")
    H, W = 1080, 1920
    gy, gx = torch.meshgrid(torch.linspace(0, 1, H, device=dev), torch.linspace(0, 1, W, device=dev), indexing="ij")
    xy = torch.stack([gx, gy], dim=-1).unsqueeze(0)
    render = torch.rand(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    dout = torch.randn(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) / (3 * H * W)
    gidx = torch.tensor([[7]], device=dev)
    result = {"tool": "bilagrid_step_time", "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup,
              "bytes_slice_fwd_min": 32 * H * W, "bytes_slice_bwd_min": 44 * H * W}

    def slice_pair(v, grids):
        r = render.clone().requires_grad_(True)
        out = SLICE[v](grids, xy, r.permute(1, 2, 0).unsqueeze(0), gidx).squeeze(0).permute(2, 0, 1)
        out.backward(dout)
        grids.grad = None

    if a.slice_only:
        grids = _grids(N_GRIDS, dev).requires_grad_(True)
        for _ in range(a.slice_only):
            slice_pair("hip", grids)
        x = _grids(N_GRIDS, dev).requires_grad_(True)
        hip_tv(x).backward()
        torch.cuda.synchronize()
        print(json.dumps({"tool": "bilagrid_step_time", "slice_only": a.slice_only, "H": H, "W": W, "n_grids": N_GRIDS}))
        return

    grids = _grids(N_GRIDS, dev).requires_grad_(True)
    result["slice_1080p"] = _alternate(lambda v: slice_pair(v, grids), a.rounds, a.steps, a.warmup)

    result["tv"] = {}
    for n in (2, 300, 2000):
        x = _grids(n, dev, seed=n).requires_grad_(True)

        def tv_pair(v):
            TV[v](x).backward()
            x.grad = None
        result["tv"][str(n)] = _alternate(tv_pair, a.rounds, a.steps, a.warmup)
        result["tv"][str(n)]["bytes_min"] = 3 * x.numel() * 4          # forward read, backward read + write
        del x
    torch.cuda.empty_cache()

    # (iii) the training step with and without the processor
    import bench_loop
    from gspl_amd import ops, optimizers
    w = T.load(a.workload, dev)
    wl, Wi, Hi, cams, order, bg, target = w.wl, w.W, w.H, w.cams, w.order, w.bg, w.target
    gy, gx = torch.meshgrid(torch.linspace(0, 1, Hi, device=dev), torch.linspace(0, 1, Wi, device=dev), indexing="ij")
    xy_w = torch.stack([gx, gy], dim=-1).unsqueeze(0)

    def model_for():
        return bench_loop.RawGaussians(*T.scene(wl, dev), active_sh_degree=3)
    variants = ("plain", "torch", "hip")
    models = {v: model_for() for v in variants}
    opts = {v: models[v].make_optimizers(1.0, optimizers.FusedAdam) for v in variants}
    bgrids = {v: _grids(N_GRIDS, dev).requires_grad_(True) for v in ("torch", "hip")}
    gopt = {v: torch.optim.Adam([bgrids[v]], lr=2e-3, eps=1e-15) for v in bgrids}
    k = [0]

    def step(v):
        g = models[v].gaussians
        ci = order[k[0] % len(order)]
        cam = cams[ci]
        k[0] += 1
        st = ops.GaussianRasterizationSettings(Hi, Wi, cam["tanfovx"], cam["tanfovy"], bg, 1.0, cam["world_to_camera"], cam["full_projection"], 3,
                                               cam["camera_center"])
        screen = torch.empty_like(g["means"]).requires_grad_(True)
        img, _ = ops.GaussianRasterizer(st)(g["means"], screen, g["opacities"], shs=g["shs_dc"], shs_rest=g["shs_rest"], scales=g["scales"],
                                            rotations=g["rotations"], raw_parameters=True)
        extra = 0
        if v != "plain":
            idx = torch.full((1, 1), ci, dtype=torch.long, device=dev)
            img = SLICE[v](bgrids[v], xy_w, img.permute(1, 2, 0).unsqueeze(0), idx).squeeze(0).permute(2, 0, 1)
            extra = 10 * TV[v](bgrids[v])
        l1, ssim = ops.l1_ssim(img.contiguous(), target)
        loss = 0.8 * l1 + 0.2 * (1 - ssim) + extra
        loss.backward()
        for o in opts[v]:
            o.step()
            o.zero_grad(set_to_none=True)
        if v != "plain":
            gopt[v].step()
            gopt[v].zero_grad(set_to_none=True)

    med, med_print, rounds_print = T.medians(T.alternate(variants, lambda v, _i: step(v), a.rounds, a.steps, a.warmup))
    result["training_step"] = {"workload": a.workload, "n_grids": N_GRIDS, "ms_median": med_print, "ms_rounds": rounds_print,
                               "processor_cost_ms": {v: round(med[v] - med["plain"], 4) for v in ("torch", "hip")}}
    print(json.dumps(result))


if __name__ == "__main__":
    main()

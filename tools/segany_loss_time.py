"""SegAnyGS behind the renderer: `gspl_amd.segany.use_hip_loss` (include/gspl_hip.h section 24) against the reference's formulation
(internal/segany_splatting.py:152-260, 317-419) restated with float32 torch ops on the same GPU, in one process, the two routes
alternating repeat by repeat.

Workload: 200 rectangular masks over a frame of `--height` x `--width` (1080p by default; run again with 540 x 960), a rendered map
[32, H, W] of the same size that requires a gradient, S ~ 1000 sampled pixels, the 10 sampled scales, learned gates.  Per route and
repeat the MEDIAN of `--steps` runs of
  step        mask preprocessing + loss forward + backward (what a training step spends behind the renderer),
  preprocess  the preprocessing alone,
  loss        the loss forward + backward alone, on one preprocessing's results,
each between its own pair of device events (host waits inside a route are part of it).  Peak device memory of each route over what was
allocated before it ran, and the kernel launches of one step as torch's profiler counts them (null where it gives none).
  python tools/segany_loss_time.py [--height 1080 --width 1920] [--steps 3] [--warmup 1] [--repeats 3] [--out profiles/segany_loss_time.json]
The result of a run is merged into `--out` under the frame's size."""
import argparse
import json
import os
import statistics
import types

import _step_time as T  # noqa: F401  (puts the repository root on sys.path)
import torch
import torch.nn.functional as F

N_MASKS, C, RAYS = 200, 32, 1000


def _median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    events = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        events.append((e0, e1))
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in events)


def restated_preprocess(self, sam_masks, mask_scales):
    """The reference's `mask_preprocess` restated: the same tensors, host waits and launches, in float32 torch."""
    with torch.no_grad():
        ub = self.upper_bound_scale
        mask_scales, order = torch.sort(mask_scales, descending=True)
        sam_masks = sam_masks.float()[order, :, :]
        n = len(mask_scales)
        index = torch.zeros(10)
        picked = torch.randperm(n)[:8]
        index[1:len(picked) + 1] = picked
        index[-1], index[0] = n - 1, -1
        index = index.long()
        scales = mask_scales[index]
        second = mask_scales[mask_scales < ub].max()
        H, W = sam_masks.shape[-2:]
        rays = torch.rand(H, W).cuda() < self.num_sampled_rays / (H * W)
        rays = torch.logical_and(rays, ~(sam_masks.sum(dim=0) == 0))
        sizes = sam_masks * sam_masks.sum(-1).sum(-1)[:, None, None]
        mean = (sizes.sum(dim=0) / (sam_masks.sum(dim=0) + 1e-9))[rays]
        pair = mean.unsqueeze(0) * mean.unsqueeze(1)
        top = pair.max()
        pair[pair == 0] = 1e10
        weight = torch.clamp(top / pair, 1.0, None)
        weight = (weight - weight.min()) / (weight.max() - weight.min()) * 9. + 1.
        sampled = sam_masks[:, rays]
        corrs = []
        scales[0] = ub + ub * torch.rand(1)[0]
        for k, si in enumerate(index):
            upper = scales[k] >= ub
            if si != n - 1 and not upper:
                scales[k] -= (scales[k] - mask_scales[si + 1]) * torch.rand(1)[0]
            elif upper:
                scales[k] -= (scales[k] - second) * torch.rand(1)[0]
            else:
                scales[k] -= scales[k] * torch.rand(1)[0]
            if not upper:
                vec = torch.zeros_like(sampled)
                vec[:si + 1, :] = sampled[:si + 1, :]
                for j in range(si, -1, -1):
                    vec[j, :] = torch.logical_and(torch.logical_not(vec[j + 1:, :].any(dim=0)), vec[j, :])
                vec[si + 1:, :] = sampled[si + 1:, :]
            else:
                vec = sampled
            corr = torch.einsum('nh,nj->hj', vec, vec)
            corr[corr != 0] = 1
            corrs.append(corr)
        return rays, weight, torch.stack(corrs, dim=0), self.q_trans(scales).squeeze()


def restated_loss(self, rendered, mask_hw, rays, weight, gt, scales):
    """The reference's loss behind `mask_preprocess` restated: the same tensors, gathers and launches, in float32 torch."""
    reg = (1 - rendered.norm(dim=0, p=2).mean()) ** 2
    rendered = F.interpolate(rendered.unsqueeze(0), mask_hw, mode='bilinear').squeeze(0)
    gates = self.scale_gate(scales.unsqueeze(-1))
    scaled = rendered.unsqueeze(0).repeat([scales.shape[0], 1, 1, 1]) * gates.unsqueeze(-1).unsqueeze(-1)
    x = F.normalize(scaled[:, :, rays].permute([0, 2, 1]), dim=-1, p=2)
    corr = torch.einsum('nhc,njc->nhj', x, x)
    diagonal = torch.eye(corr.shape[1], dtype=torch.bool, device=corr.device)
    total = gt.sum(dim=0)
    negative, positive = total == 0, total == len(gt)
    mixed = torch.logical_not(torch.logical_or(negative, positive))
    half = mixed.count_nonzero() / 2
    draw = torch.rand_like(total)
    keep_pos = torch.logical_and(positive, draw < half / positive.count_nonzero())
    keep_neg = torch.logical_and(negative, draw < half / negative.count_nonzero())
    m_pos = torch.logical_or(torch.logical_or(keep_pos, torch.any(torch.logical_and(corr < 0.75, gt == 1), dim=0)), mixed)
    m_pos = torch.triu(torch.logical_and(m_pos, ~diagonal), diagonal=0).bool()
    m_neg = torch.logical_or(torch.logical_or(keep_neg, torch.any(torch.logical_and(corr > 0.5, gt == 0), dim=0)), mixed)
    m_neg = torch.triu(torch.logical_and(m_neg, ~diagonal), diagonal=0).bool()
    weight = weight.unsqueeze(0)
    loss = (-weight[:, m_pos] * gt[:, m_pos] * corr[:, m_pos]).mean() \
        + (weight[:, m_neg] * (1 - gt[:, m_neg]) * torch.relu(corr[:, m_neg])).mean() + self.rfn * reg
    with torch.no_grad():
        return loss, corr[gt == 1].mean(), corr[gt == 0].mean()


def _frame(H, W, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    masks = torch.zeros(N_MASKS, H, W, dtype=torch.bool, device=dev)
    for i in range(N_MASKS):
        h, w = int(torch.randint(H // 20, H // 2, (1,), generator=gen)), int(torch.randint(W // 20, W // 2, (1,), generator=gen))
        y, x = int(torch.randint(0, H - h, (1,), generator=gen)), int(torch.randint(0, W - w, (1,), generator=gen))
        masks[i, y:y + h, x:x + w] = True
    scales = (masks.flatten(1).sum(1).float().sqrt() * (0.9 + 0.2 * torch.rand(N_MASKS, generator=gen).to(dev)))
    return masks, scales, torch.randn(C, H, W, generator=gen).to(dev)


def _launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        count = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return count or None
    except Exception:
        return None


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--height", type=int, default=1080)
    p.add_argument("--width", type=int, default=1920)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--no-launch-count", action="store_true")
    p.add_argument("--out", default=os.path.join(T.ROOT, "profiles", "segany_loss_time.json"))
    a = p.parse_args()
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    from gspl_amd.segany import _hip_preprocess, use_hip_loss
    assert torch.cuda.is_available(), "segany_loss_time measures on the GPU"
    dev = torch.device("cuda:0")
    H, W = a.height, a.width
    masks, scales, rendered_values = _frame(H, W, dev, 42)
    torch.manual_seed(1)
    gate = torch.nn.Sequential(torch.nn.Linear(1, C, bias=True), torch.nn.Sigmoid()).to(dev)

    class Module(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.scale_gate = gate
            self.upper_bound_scale, self.ray_sample_rate, self.num_sampled_rays = float(scales.max()), 0, RAYS
            self.scale_aware_dim, self.rfn = -1, 1.0
            self.q_trans = lambda s: (s / (1 + s)).reshape(-1, 1)
            self.rendered = None

        def forward(self, camera):
            return {"render": self.rendered}

    hip, ref = use_hip_loss(Module()), Module()
    pre = types.SimpleNamespace()

    def leaf():
        return rendered_values.detach().requires_grad_(True)

    def hip_step():
        hip.rendered = leaf()
        hip.forward_with_loss_calculation(None, None, (masks, scales))[1].backward()

    def ref_step():
        r = leaf()
        restated_loss(ref, r, (H, W), *restated_preprocess(ref, masks, scales))[0].backward()

    def hip_pre():
        pre.hip = _hip_preprocess(hip, masks, scales)

    def ref_pre():
        pre.ref = restated_preprocess(ref, masks, scales)

    def hip_loss():
        s, r = pre.hip, leaf()
        gates = gate(s.sampled_scales.unsqueeze(-1))
        rand = torch.rand((s.pixel_index.numel(),) * 2, device=dev)
        loss = ops.segany_correspondence_loss(r, s.mask_hw, s.pixel_index, gates, s.labels, s.counts, s.a, rand)[0]
        (loss + (1 - r.norm(dim=0, p=2).mean()) ** 2).backward()

    def ref_loss():
        restated_loss(ref, leaf(), (H, W), *pre.ref)[0].backward()

    hip_pre(), ref_pre()
    routes = {"restated": {"step": ref_step, "preprocess": ref_pre, "loss": ref_loss}, "kernel": {"step": hip_step, "preprocess": hip_pre, "loss": hip_loss}}
    medians = {name: {part: [] for part in parts} for name, parts in routes.items()}
    peaks = {name: 0 for name in routes}
    for rep in range(a.repeats):
        for name in (list(routes) if rep % 2 == 0 else list(routes)[::-1]):
            for part, fn in routes[name].items():
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                before = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                medians[name][part].append(_median_ms(fn, a.steps, a.warmup))
                if part == "step":
                    peaks[name] = max(peaks[name], torch.cuda.max_memory_allocated() - before)
    launches = {name: None if a.no_launch_count else _launches(parts["step"]) for name, parts in routes.items()}
    result = {
        "tool": "segany_loss_time", "masks": N_MASKS, "frame": [H, W], "C": C, "scales": 10, "sampled_pixels": int(pre.hip.pixel_index.numel()),
        "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
        "ms_repeats": {name: {part: [round(x, 3) for x in v] for part, v in parts.items()} for name, parts in medians.items()},
        "ms_median_of_repeats": {name: {part: round(statistics.median(v), 3) for part, v in parts.items()} for name, parts in medians.items()},
        "kernel_faster_beyond_spread": {part: max(medians["kernel"][part]) < min(medians["restated"][part]) for part in ("step", "preprocess", "loss")},
        "peak_bytes_over_inputs": peaks, "peak_ratio_restated_over_kernel": round(peaks["restated"] / max(peaks["kernel"], 1), 2),
        "launches_per_step": launches,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    merged = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            merged = json.load(f)
    merged[f"{H}x{W}"] = result
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""
bench.py — headline benchmark of the rasterizer hot path (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload S-1080p-1M] [--api vanilla|gsplat]
                    [--parallelism auto|single|replicated|sharded] [--optimizer fused-adam|none|...] [--dump-outputs DIR]

A "step" is one TRAINING step over one camera of synthetic input: renderer forward (preprocess + SH + binning +
compositing), the reference's photometric loss, the full backward down to the activated Gaussian properties (means,
scales, rotations, opacities, SH), the optimizer step (fused Adam by default) and the density controller's statistics
update.  Inputs are resident in HBM before the timed region.  `value` = images/s over all ranks with the optimizer
step inside the timed region; the same line also carries `images_per_s_renderer_only` (forward + loss + backward +
statistics, no parameter update — what round 1 reported as `value`), measured in a second timed region of the same run
(N = 1 only).

Multi-GPU (driver launches `torch.distributed.run ... bench.py --gpus N`), one process per GPU over RCCL, one camera per
rank per step (weak scaling):
  sharded     (default for N > 1; the reference's configs/distributed.yaml, SURVEY.md §8e "primary"): Gaussians sharded over
              the ranks, every rank projects its shard for all N cameras, one packed all-to-all of visible-splat records
              (48 B per visible splat), compositing local (gspl_amd.renderers.HipGSplatDistributedRenderer), optimizer and
              statistics on the shard: no gradient all-reduce.
  replicated  (BASELINE.json north_star's wording, the reference's configs/ddp.yaml): every rank holds all Gaussians;
              parameter gradients are all-reduced (averaged; 236 B per Gaussian per step: bound by the xGMI links at 1 M
              Gaussians) before the optimizer step, the densification statistics (12 B/Gaussian) every 100 steps (the
              reference's cadence) and at the end of the timed region.

Extra objects on the JSON line:
  roofline      dominant kernel = composite backward; achieved = algorithmic bytes (76*I + 20*P, SURVEY.md §8d, I = every
                tile-rect intersection of the API benched) / its mean launch duration measured with HIP events inside the
                timed steps; peak = 8000 GB/s (MI355X_MICROARCH.md).  Also: `list_entries` (I', what the kernel actually
                walks after lossless tile culling) with the fraction computed on it, `valid_pairs` ((pixel, splat) pairs
                COUNTED on the device for this frame) and `valu_frac` = 70 flop per counted pair / time / 157.3 TFLOP/s,
                `traffic` = PMC-measured HBM bytes per launch with `traffic_source` naming the profile it was read from.
  cpu_baseline  host-core baseline, rank 0, N = 1 only, one bounded pass: kind "port" = the oracle (torch fp32
                projection + SH restating the reference's Python + the OpenMP C compositing loops); when the reference tree
                is importable (GSPL_REFERENCE_ROOT, default /root/reference) its own project_gaussians + eval_sh are
                timed as well (`reference_projection_sh`, kind "reference").  `--cpu-baseline-only` runs just this leg
                (no GPU needed).
"""
import os as _os
_os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: what RCCL / tensor sharing need on this driver

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md "HBM3E peak BW"
FP32_PEAK_TFLOPS = 157.3       # vector fp32


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--cameras", type=int, default=16,
                   help="size of the synthetic camera set the steps cycle through (one camera per rank per step, as the reference's data "
                        "loader hands them out, internal/dataset.py:146-184); 1 = the fixed camera of rounds 1-2")
    p.add_argument("--cameras-set", default="heterogeneous", choices=["heterogeneous", "orbit"],
                   help="heterogeneous (default since round 6): views at 0.55-1.75 x the workload's distance — list lengths spread 2.9 x around the orbit "
                        "set's mean — served in a fresh random permutation every epoch, as the reference's loader serves a capture "
                        "(internal/dataset.py:216-217); orbit: the near-identical views of rounds 3-5 (+-22 % in list length) in set order")
    p.add_argument("--no-stage-rooflines", action="store_true", help="skip the staged pass that times every stage for `stage_rooflines`")
    p.add_argument("--no-workload-stats", action="store_true",
                   help="skip the per-camera pass that counts I, I', V and the blended pairs after the timed regions (profiler runs: the last "
                        "launches of the process are then the last timed step); the line carries no roofline")
    p.add_argument("--workload", default="S-1080p-1M")
    p.add_argument("--api", default=None, choices=["vanilla", "gsplat"], help="default: the workload's (vanilla unless it says otherwise)")
    p.add_argument("--loss", default="photometric", choices=["l1", "photometric"],
                   help="l1: mean |render - target| with torch ops; photometric: the reference's training loss "
                        "0.8 L1 + 0.2 (1 - SSIM) (vanilla_metrics.py:66-68) through the fused HIP loss kernels")
    p.add_argument("--optimizer", default="fused-adam", choices=["none", "fused-adam", "fused-bwd-adam", "selective-adam", "torch-adam", "masked-adam"],
                   help="optimizer step inside the timed step (default: the package's fused Adam; none = renderer fwd+bwd rate only; "
                        "masked-adam: --parallelism replicated with the visibility-masked reduce-scatter / all-gather and the optimizer "
                        "state sharded by row ownership, distributed.MaskedReplicaAdam)")
    p.add_argument("--parallelism", default="auto", choices=["auto", "single", "replicated", "sharded"],
                   help="auto: single for one GPU, sharded for several (Gaussian-sharded renderer with the packed all-to-all, "
                        "configs/distributed.yaml); replicated: all Gaussians on every rank, gradient all-reduce + optimizer on every rank")
    p.add_argument("--overlap-sh-update", action="store_true",
                   help="run the shs_rest update on the colour stream, under the next frame's geometry + binning (FusedAdam(deferred=...), "
                        "HipFusedAdam.overlap_sh_update=True).  Off by default, as in the product: the headline number is the default configuration")
    p.add_argument("--no-overlap-sh-update", action="store_true", help="(the default; kept for older command lines)")
    p.add_argument("--exchange", default="auto", choices=["counted", "padded", "auto"],
                   help="--parallelism sharded: format of the per-step record exchange (renderer option `exchange`)")
    p.add_argument("--exchange-transport", default="auto", choices=["auto", "collective", "peer"],
                   help="--parallelism sharded: collective = torch.distributed all-to-all (RCCL); peer = direct writes into the peers' IPC-mapped "
                        "receive buffers + flags (renderer option `exchange_transport`).  auto (default): collective with one rank; with several, "
                        "peer IF it sets up on every rank and one validation frame equals the collective route's image bit for bit on every "
                        "rank, else collective")
    p.add_argument("--staged-sharded-step", action="store_true",
                   help="--parallelism sharded: the stage-by-stage formulation of the step (eleven autograd nodes) instead of the three-node one")
    p.add_argument("--no-renderer-only", action="store_true", help="skip the second timed region (no optimizer) of a one-GPU run")
    p.add_argument("--loop", default="reference-shaped", choices=["none", "reference-shaped"],
                   help="one-GPU runs: after the timed regions, also run the REFERENCE-SHAPED training loop (bench_loop.py: raw parameters "
                        "behind exp / sigmoid / normalize getters, the restated density controller densifying every 100 steps from the "
                        "workload's Gaussians, opacity reset, SH-degree raise, the renderer plugin) and report `reference_shaped_loop`")
    p.add_argument("--loop-steps", type=int, default=450)
    p.add_argument("--no-loop-comparison", action="store_true", help="skip the second run of the reference-shaped loop (activations left to torch)")
    p.add_argument("--cpu-baseline-only", action="store_true", help="run only the CPU baseline leg and print it (no GPU needed)")
    p.add_argument("--stage-times", action="store_true",
                   help="time EVERY C-ABI call with events (stages_ms); default: only the compositing kernels the roofline needs")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--cpu-sample", default="auto", help="workload name for the CPU baseline leg, or 'auto'")
    p.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL; default) or gloo (code-path test on one GPU)")
    p.add_argument("--share-device", action="store_true", help="testing only: every rank uses cuda:0")
    p.add_argument("--init-dist", action="store_true",
                   help="testing only: with --gpus 1, create a process group of ONE rank and issue every collective of the chosen "
                        "--parallelism anyway (the RCCL code paths on a one-GPU machine)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed step computed (rank 0: rendered image, loss, radii, the "
                        "viewspace gradient, the updated parameters and their gradients, the densification statistics) as "
                        "DIR/<name>.npy, float32 / float64, at most 64 MB in all (per-Gaussian arrays: a fixed seeded sample of rows)")
    return p.parse_args()


def entries_walked(last, W, H, tile=16):
    """List entries the compositing kernels WALK in this frame: per tile, from the head of its list to the deepest entry any of its
    pixels blended (`last_ids` = one past it; the backward starts there, the forward stops within a round of it).  In a scene that
    saturates this is far below the list length — the byte model is priced on it, not on entries the kernels never read."""
    li, offs = last["last_ids"], last["offsets"]
    th, tw = (H + tile - 1) // tile, (W + tile - 1) // tile
    pad = torch.zeros((th * tile, tw * tile), dtype=li.dtype, device=li.device)
    pad[:H, :W] = li
    deepest = pad.view(th, tile, tw, tile).amax(dim=(1, 3)).reshape(-1)
    return int((deepest - offs[:th * tw]).clamp_min(0).sum(dtype=torch.int64).item())


def _mark():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def reference_shaped_loop(dev, wl, cam_dicts, steps, fuse_activations=True, prewarm=False, fuse_optimizer=False, view_stream=None, per_step=False):
    """`--loop reference-shaped` (images/s of the Lightning loop, not of a static-N step on activated leaves): the
    consumer side restated in bench_loop.py drives `HipVanillaRenderer` through what `GaussianSplatting.training_step` does
    (internal/gaussian_splatting.py:329-397) — raw parameters behind exp / normalize / sigmoid getters (fuse_activations: evaluated
    inside the renderer's preprocess kernels, the plugin's default for such a model; False: by torch around it, forward and backward
    every step, as the reference's renderer has them), densify / prune every 100 steps (N changes: allocator, list-length guesses
    and optimizer state see new sizes), one opacity reset, the SH degree raised twice."""
    import bench_loop as BL
    import gspl_amd  # noqa: F401
    from gspl_amd import ops, synthetic
    from gspl_amd.optimizers import FusedAdam
    from gspl_amd.renderers import HipVanillaRenderer
    W, H = wl["width"], wl["height"]
    cams = [synthetic.CameraObject(c, dev, idx=i) for i, c in enumerate(cam_dicts)]
    renderer = HipVanillaRenderer(fuse_activations=fuse_activations)
    bg = torch.zeros(3, device=dev)
    loss_fn = lambda img, gt: ops.photometric_loss(img, gt, 0.2)

    def setup(n, from_iter, interval, reset):
        clean = (synthetic.scene_surfaces if wl.get("scene") == "surfaces" else synthetic.scene)(n, seed=42)
        # targets: the clean scene from every camera (degree 3); the trained model starts from a perturbed copy at degree 1
        truth = synthetic.ModelObject(*[t.to(dev) for t in clean], active_sh_degree=3)
        with torch.no_grad():
            targets = [renderer(c, truth, bg)["render"].clone() for c in cams]
        model = BL.RawGaussians(*[t.to(dev) for t in BL.perturbed(clean)], active_sh_degree=1, max_sh_degree=3)
        controller = BL.DensityController(model.n_gaussians, dev, cameras_extent=2.6, densify_from_iter=from_iter, densification_interval=interval,
                                          opacity_reset_interval=reset)
        # fuse_optimizer: both optimizers built with fuse_into_backward=True — the rasterizer's backward applies their updates (the
        # parameters of the two optimizers are claimed together, the densification surgery's new Parameters are found by address)
        return targets, model, model.make_optimizers(1.0, FusedAdam, **({"fuse_into_backward": True} if fuse_optimizer else {})), controller

    if prewarm:
        # the torch kernels of a densification event (mask gathers, cats, multinomial-free split sampling ...) are loaded on first use
        # — hundreds of milliseconds once per process, which belong to neither run of the loop: a 20 k-Gaussian model goes through
        # two events and an opacity reset first, untimed
        t_, m_, o_, c_ = setup(20_000, 40, 40, 80)
        BL.run(renderer, m_, c_, o_, cams, t_, 90, bg, loss_fn, sh_degree_up_interval=45)
        del t_, m_, o_, c_
    torch.cuda.empty_cache()          # every run of the loop starts with a cold caching allocator (the event steps' device mallocs are part of it)
    # the reference's defaults (vanilla_density_controller.py:14-40) except the schedule, compressed so that a few hundred steps see
    # every kind of event: densification from step 100 every 100 steps (reference: from 500), opacity reset at step 300 (3000),
    # SH degree up every 150 steps (1000)
    targets, model, optimizers, controller = setup(wl["n"], 100, 100, 300)
    frames0, misses0, cold0 = (ops.SPECULATION[k] for k in ("frames", "misses", "cold"))
    mallocs0 = torch.cuda.memory_stats(dev).get("num_device_alloc", 0)
    # per_step (the attribution run): host-side counters after every step — the caching allocator's hipMalloc count, the
    # speculation's cold / missed frames, N and the SH degree — to say what the steps after a densification event or an SH-degree raise pay for
    trace, comp = [], {}
    RESET_STEP = 300
    def on_step(step, outputs):
        trace.append((torch.cuda.memory_stats(dev).get("num_device_alloc", 0), ops.SPECULATION["misses"], ops.SPECULATION["cold"],
                      model.n_gaussians, model.active_sh_degree))
        if step == RESET_STEP:      # the compositing launches' durations up to the opacity reset and after it, apart (one synchronisation, traced run only)
            comp["before_reset"] = _lib.profile_stop()
            _lib.profile_start(("gspl_composite_bwd_packed", "gspl_composite_fwd"), period=1)
    if per_step:
        from gspl_amd import _lib
        _lib.profile_start(("gspl_composite_bwd_packed", "gspl_composite_fwd"), period=1)
    res = BL.run(renderer, model, controller, optimizers, cams, targets, steps, bg, loss_fn, sh_degree_up_interval=150, view_stream=view_stream,
                 on_step=on_step if per_step else None)
    if per_step:
        comp["after_reset" if "before_reset" in comp else "before_reset"] = _lib.profile_stop()
    event_steps = {e["step"] for e in controller.events}
    quiet = [ms for i, ms in enumerate(res["step_ms"], start=1) if i not in event_steps and (i - 1) not in event_steps and i > 5]
    loud = [ms for i, ms in enumerate(res["step_ms"], start=1) if i in event_steps]
    srt = sorted(quiet)
    attribution = None
    if per_step and trace:
        # where the mean exceeds the quiet median: every step's excess over the quiet p50, binned by what preceded it
        p50 = srt[len(srt) // 2] if srt else 0.0
        sh_steps = {s_ for s_ in range(150, steps + 1, 150)}
        AFTER_RESET = "steps after the opacity reset (every opacity at 0.01: no pixel saturates, the compositing kernels walk the whole lists)"
        rows, bins = [], {"event steps": 0.0, AFTER_RESET: 0.0, "1-10 steps after an event": 0.0, "1-10 steps after an SH-degree raise": 0.0,
                          "steps 1-5 of the loop": 0.0, "every other step": 0.0}
        prev = (mallocs0, misses0, cold0, None, None)
        for i, ms in enumerate(res["step_ms"], start=1):
            cur = trace[i - 1]
            d_malloc, d_miss, d_cold = cur[0] - prev[0], cur[1] - prev[1], cur[2] - prev[2]
            prev = cur
            since_event = min((i - e for e in event_steps if e <= i), default=None)
            since_sh = min((i - e for e in sh_steps if e < i), default=None)
            excess = ms - p50
            if i in event_steps:
                key = "event steps"
            elif i > RESET_STEP:
                key = AFTER_RESET
            elif since_event is not None and 1 <= since_event <= 10:
                key = "1-10 steps after an event"
            elif since_sh is not None and 1 <= since_sh <= 10:
                key = "1-10 steps after an SH-degree raise"
            elif i <= 5:
                key = "steps 1-5 of the loop"
            else:
                key = "every other step"
            bins[key] += excess
            if (key not in ("every other step", AFTER_RESET)) or d_malloc or d_miss or d_cold or (key == "every other step" and excess > 0.25):
                rows.append({"step": i, "ms": round(ms, 3), "excess_ms": round(excess, 3), "what": key if key != AFTER_RESET else "after the opacity reset",
                             "device_mallocs": d_malloc, "misses": d_miss, "cold": d_cold, "n": cur[3], "sh_degree": cur[4]})
        total_excess = sum(ms - p50 for ms in res["step_ms"])
        mean_of = lambda pr, k: round(sum(pr.get(k, [])) / max(len(pr.get(k, [])), 1), 4) if pr.get(k) else None
        attribution = {"what": "sum over the loop's steps of (step time - the quiet median), binned by what the step follows; the traced run reads host-side counters "
                               "after every step and synchronises once (at the reset step), its own rate is not reported",
                       "quiet_p50_ms": round(p50, 4), "total_excess_ms": round(total_excess, 2), "excess_ms_by_cause": {k: round(v, 2) for k, v in bins.items()},
                       "explained_share": round(1.0 - abs(bins["every other step"]) / max(total_excess, 1e-9), 3),
                       "compositing_ms_per_step": {w: {"fwd": mean_of(pr, "gspl_composite_fwd"), "bwd": mean_of(pr, "gspl_composite_bwd_packed")} for w, pr in comp.items()},
                       "steps": rows}
    return {
        "attribution": attribution,
        "what": "bench_loop.py: RawGaussians (exp / sigmoid / normalize getters) + restated VanillaDensityControllerImpl + FusedAdam x 2 "
                "+ HipVanillaRenderer + fused 0.8 L1 + 0.2 (1 - SSIM), one camera of the set per step, targets = the unperturbed scene",
        "activations": ("inside the preprocess kernels (HipVanillaRenderer.fuse_activations, renderer.model_raw_parameters)" if fuse_activations
                        else "torch getters around the renderer, forward and backward (fuse_activations=False)"),
        "steps": steps, "images_per_s_densifying": round(steps / res["elapsed_s"], 2), "ms_per_step_mean": round(1e3 * res["elapsed_s"] / steps, 4),
        "ms_per_step_between_events_p50": round(srt[len(srt) // 2], 4) if srt else None,
        "ms_per_event_step_mean": round(sum(loud) / len(loud), 3) if loud else None,
        "n_start": res["n"][0] if res["n"] else None, "n_end": res["n"][-1] if res["n"] else None,
        "n_trajectory_every_50_steps": res["n"][49::50], "events": controller.events,
        "sh_degree_end": model.active_sh_degree, "loss_first_last": [round(res["loss"][0], 5), round(res["loss"][-1], 5)],
        "speculation": {"frames": ops.SPECULATION["frames"] - frames0, "misses": ops.SPECULATION["misses"] - misses0,
                        "cold": ops.SPECULATION["cold"] - cold0},
        "device_mallocs": torch.cuda.memory_stats(dev).get("num_device_alloc", 0) - mallocs0,
        "schedule": {"densify_from_iter": 100, "densification_interval": 100, "opacity_reset_interval": 300, "sh_degree_up_interval": 150,
                     "densify_grad_threshold": 0.0002, "reference_defaults": "500 / 100 / 3000 / 1000 / 0.0002"},
    }


def make_step(api, dev, wl, cams, tensors, loss_kind="l1", rank=0, world=1, stream=None):
    """One training step (forward, loss, backward) on the next camera of `cams`: call k of rank r takes position k * world + r of the
    job's view stream (`stream`: synthetic.ViewStream — a fresh permutation of the set per epoch; None: set order, cyclically).  With
    state["marks"] = [] the step leaves three events per call (start, before backward, after backward) for the fwd_ms / bwd_ms of the
    bench line."""
    sh_degree, absgrad = wl.get("sh_degree", 3), bool(wl.get("absgrad", False))
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    # the reference model's six parameters (shs_dc and shs_rest apart, vanilla_gaussian.py:266-300); five at SH degree 0
    m, s, q, o, dc = tensors[:5]
    rest = tensors[5] if len(tensors) > 5 else None
    W, H = wl["width"], wl["height"]
    bg = torch.zeros(3, device=dev)
    target = torch.full((3, H, W), 0.5, device=dev)
    state = {"k": 0}
    if loss_kind == "photometric":
        loss_fn = lambda img: ops.photometric_loss(img, target, 0.2)
    else:
        loss_fn = lambda img: (img - target).abs().mean()

    def next_camera():
        pos = state["k"] * world + rank
        i = stream.view(pos) if stream is not None else pos % len(cams)
        state["k"] += 1
        state["camera"] = i
        return i
    if api == "vanilla":
        from gspl_amd.density import request_stats_in_backward
        # the cameras' device tensors are made ONCE per camera dictionary (a data set's cameras are persistent: the per-camera pass and the
        # timed steps see the same view matrices — what the rasterizer's per-view memory of the segmented backward is keyed on)
        for cam in cams:
            if "_device_tensors" not in cam or cam["_device_tensors"][0] != str(dev):
                cam["_device_tensors"] = (str(dev), cam["world_to_camera"].to(dev), cam["full_projection"].to(dev), cam["camera_center"].to(dev))
        rasts = [ops.GaussianRasterizer(ops.GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=bg, scale_modifier=1.0,
            viewmatrix=cam["_device_tensors"][1], projmatrix=cam["_device_tensors"][2], sh_degree=sh_degree,
            campos=cam["_device_tensors"][3])) for cam in cams]

        def step():
            for t in tensors:
                t.grad = None
            rast = rasts[next_camera()]
            marks = state.get("marks")
            if marks is not None:
                marks.append(_mark())
            screen = torch.empty_like(m).requires_grad_(True)      # gradient carrier, as HipVanillaRenderer creates it (values unused)
            render, radii = rast(means3D=m, means2D=screen, opacities=o, shs=dc, shs_rest=rest, scales=s, rotations=q)
            loss = loss_fn(render)
            # HipDensityStatsMixin.before_backward: the statistics' buffers go to the frame's backward (density.py), which applies the
            # update of densification_stats() below itself; `state["stats_buffers"]` is set by the steps that keep statistics
            bufs = state.get("stats_buffers")
            state["stats_request"] = request_stats_in_backward(radii, *bufs) if bufs is not None else None
            if marks is not None:
                marks.append(_mark())
            loss.backward()
            if marks is not None:
                marks.append(_mark())
            state["vs_grad"], state["radii"], state["loss"] = screen.grad, radii, loss
            state["grad_scale"] = None
            if state.get("keep_render"):          # --dump-outputs only
                state["render"] = render.detach()
            return state
    else:
        vms = [cam["world_to_camera"].T.contiguous().to(dev) for cam in cams]
        centers = [cam["camera_center"].to(dev) for cam in cams]
        grad_scale = torch.tensor([0.5 * W, 0.5 * H], device=dev)      # what the renderers return as viewspace_points_grad_scale

        def step():
            for t in tensors:
                t.grad = None
            i = next_camera()
            cam, vm, center = cams[i], vms[i], centers[i]
            marks = state.get("marks")
            if marks is not None:
                marks.append(_mark())
            xys, depths, radii, conics, comp, tiles, _ = ops.project_gaussians(
                m, s, 1.0, q, vm[:3], cam["fx"], cam["fy"], cam["cx"], cam["cy"], H, W, 16, return_cov3d=False)
            xys.retain_grad()
            opac = o * comp[:, None]
            # same order as HipGSplatRenderer.forward: count half of the binning, SH, emit half, compositing
            pending = ops.bin_gaussians_begin(xys, depths, radii, H, W, 16, conics=conics, opacities=opac)
            rgbs = ops.sh_view_colors(sh_degree, m, center, dc, rest, radii > 0)
            img = ops.rasterize_gaussians(xys, depths, radii, conics, tiles, rgbs, opac, H, W, 16, bg, absgrad=absgrad,
                                          isects=ops.bin_gaussians_end(pending, lazy=True), channels_first=True)
            loss = loss_fn(img)
            if marks is not None:
                marks.append(_mark())
            loss.backward()
            if marks is not None:
                marks.append(_mark())
            # configs/gsplat-absgrad.yaml:6-8: the density controller reads `viewspace_points.absgrad`
            state["vs_grad"], state["radii"], state["loss"] = (xys.absgrad if absgrad else xys.grad), radii, loss
            state["grad_scale"] = grad_scale
            if state.get("keep_render"):          # --dump-outputs only
                state["render"] = img.detach()
            return state
    step.state = state
    return step


def densification_stats(state, accum, denom, max_radii):
    """What VanillaDensityControllerImpl.update_states accumulates
    (internal/density_controllers/vanilla_density_controller.py:101-123), on the fused kernel the package ships for it
    (gspl_amd.density.HipDensityStatsMixin): masked max of the radii, masked sum of the scaled gradient norms, masked count."""
    from gspl_amd.density import update_densification_stats, withdraw_stats_request
    req = state.pop("stats_request", None)
    withdraw_stats_request(req)
    if req is not None and req.applied:       # HipDensityStatsMixin.update_states: this frame's backward has applied them
        return
    update_densification_stats(state["vs_grad"], None, state["radii"], accum, denom, max_radii, scale=state["grad_scale"])


DUMP_BYTES_MAX = 64 << 20      # --dump-outputs: all files together
DUMP_ROWS = 32768              # per-Gaussian arrays: at most this many rows (a fixed seeded sample, in row order)
DUMP_IMAGE_VALUES = 8 << 20    # a larger image: this many of its values (a fixed seeded sample, in index order)


def dump_outputs(out_dir, state, named_leaves, stats, after_step):
    """--dump-outputs: what the last timed step computed, as the caller of the step receives it, one float32 / float64 .npy file per
    array.  The inputs are seeded, so two builds run with the same arguments can be compared file by file; the samples (rows of the
    per-Gaussian arrays, values of an image too large to keep whole) are drawn from fixed seeds and are the same in every run with the
    same workload.  `gaussian_rows.npy` names the rows kept; `after_step` (the result line) counts the steps taken, warm-up included."""
    import numpy as np
    arrays = {}
    n = named_leaves[0][1].shape[0]
    rows = None
    if n > DUMP_ROWS:
        rows = torch.randperm(n, generator=torch.Generator().manual_seed(1234))[:DUMP_ROWS].sort().values
        arrays["gaussian_rows"] = rows.double()

    def host(t, per_row=False):
        t = t.detach()
        if per_row and rows is not None:
            t = t[rows.to(t.device)]
        return t.cpu().double() if t.dtype == torch.float64 else t.cpu().float()

    out = state.get("out")                   # the sharded step keeps the renderer's output dictionary
    render = out["render"] if out is not None else state["render"]
    if render.numel() > DUMP_IMAGE_VALUES:
        keep = torch.randperm(render.numel(), generator=torch.Generator().manual_seed(4321))[:DUMP_IMAGE_VALUES].sort().values
        arrays["render_sample"] = host(render.reshape(-1)[keep.to(render.device)])
    else:
        arrays["render"] = host(render)
    arrays["loss"] = state["loss"].detach().cpu().double().reshape(())
    if out is not None:                      # one entry per camera of the step, over this rank's rows
        arrays["radii"] = torch.stack([host(r[0], True) for r in out["projection_results_list"]], dim=1)
        grads = [r[1].grad for r in out["projection_results_list"]]
        if all(g is not None for g in grads):
            arrays["viewspace_grad"] = torch.stack([host(g, True) for g in grads], dim=1)
    else:
        arrays["radii"] = host(state["radii"], True)
        if state.get("vs_grad") is not None:
            arrays["viewspace_grad"] = host(state["vs_grad"], True)
    for name, t in named_leaves:
        arrays["param_" + name] = host(t, True)
        if t.grad is not None:
            arrays["grad_" + name] = host(t.grad, True)
    for name, t in stats:
        arrays["stats_" + name] = host(t, True)
    total = sum(a.numel() * a.element_size() for a in arrays.values())
    assert total <= DUMP_BYTES_MAX, f"--dump-outputs: {total} bytes (cap {DUMP_BYTES_MAX})"
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a.numpy())
    return {"dir": out_dir, "after_step": after_step, "bytes": total, "rows_of": n, "rows_kept": n if rows is None else int(rows.numel()),
            "files": {name: list(a.shape) for name, a in arrays.items()}}


def cpu_baseline(workload_name, api):
    """Oracle port timed on the host cores (one bounded pass; fp32; all threads)."""
    import numpy as np
    from gspl_amd import synthetic
    from oracle import gsplat_oracle as O
    wl = synthetic.WORKLOADS[workload_name]
    # elementwise torch ops degrade badly when oversubscribed (28 s vs ~1 s for the projection on a
    # 256-thread host), so the baseline uses at most 32 threads and reports that number
    cores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(cores)
    os.environ["OMP_NUM_THREADS"] = str(cores)
    means, scales, quats, opac, shs = synthetic.workload_scene(wl, seed=42)
    cam = synthetic.camera(wl["width"], wl["height"], wl["fx"])
    W, H = wl["width"], wl["height"]
    leaves = [t.clone().requires_grad_(True) for t in (means, scales, quats, opac, shs)]
    m, s, q, o, c = leaves
    lib = O._lib()
    import ctypes
    lib.oracle_set_threads(ctypes.c_int(cores))

    t0 = time.perf_counter()
    xys, depths, radii, conics, comp, n_tiles, _, mask, _, _ = O.project_gaussians(
        m, s, 1.0, q, cam["world_to_camera"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], H, W)
    rgbs = O.sh_colors(3, c, m, cam["camera_center"], detach_dirs=True)
    op = o.reshape(-1) * comp
    t1 = time.perf_counter()
    tiles, ids, flat, offs = O.isect_tiles(O.MODE_GSPLAT, xys, radii, depths, W, H)
    t2 = time.perf_counter()
    f = lambda t: np.ascontiguousarray(t.detach().numpy(), np.float32)
    a_xy, a_con, a_col, a_op = f(xys), f(conics), f(rgbs), f(op)
    bg = np.zeros(3, np.float32)
    tw, th = (W + 15) // 16, (H + 15) // 16
    out = np.empty((H, W, 3), np.float32)
    alpha = np.empty((H, W), np.float32)
    last = np.empty((H, W), np.int32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lib.oracle_composite_fwd_f32(ctypes.c_int(0), ctypes.c_int64(flat.shape[0]), ctypes.c_int(3), P(a_xy), P(a_con), P(a_col),
                                 P(a_op), P(bg), ctypes.c_int(W), ctypes.c_int(H), ctypes.c_int(tw), ctypes.c_int(th),
                                 P(offs), P(flat), P(out), P(alpha), P(last))
    t3 = time.perf_counter()
    v_out = (np.sign(out - 0.5) / out.size).astype(np.float32)
    g_xy, g_con, g_col, g_op = (np.zeros_like(a) for a in (a_xy, a_con, a_col, a_op))
    lib.oracle_composite_bwd_f32(ctypes.c_int(0), ctypes.c_int(wl["n"]), ctypes.c_int64(flat.shape[0]), ctypes.c_int(3),
                                 P(a_xy), P(a_con), P(a_col), P(a_op), P(bg), ctypes.c_int(W), ctypes.c_int(H),
                                 ctypes.c_int(tw), ctypes.c_int(th), P(offs), P(flat), P(alpha), P(last), P(v_out),
                                 P(g_xy), P(g_con), P(g_col), P(g_op))
    t4 = time.perf_counter()
    torch.autograd.backward([xys, conics, rgbs, op],
                            [torch.from_numpy(g_xy), torch.from_numpy(g_con), torch.from_numpy(g_col), torch.from_numpy(g_op)])
    t5 = time.perf_counter()
    # `value`: the legs a CPU implementation of this path would spend its time in — projection + SH (torch, all cores) and the
    # compositing pair (C, OpenMP).  The binning leg between them is the ORACLE's numpy restatement of the key sort (test
    # infrastructure, single-threaded sort of 13.8 M 64-bit keys): timed and listed, but nobody would ship it, so it stays out of
    # `value` and `value_with_numpy_binning` carries the figure rounds 1-3 reported.
    binning_s = t2 - t1
    total = (t5 - t0) - binning_s
    ref = None
    try:
        ref = reference_projection_sh(workload_name, cores)
    except Exception as e:      # the reference leg is optional evidence
        ref = {"kind": "reference", "failed": repr(e)}
    # The reference's OWN figures in short keys the driver's `parsed.cpu_baseline` keeps (VERDICT r5 #8a): measured live where the
    # reference tree exists, else the constant measured in the 8-vCPU build container (S-1080p-1M only).  The PORT is not a timing
    # proxy for them: its projection + SH backward is ~5 x faster than the reference's own autograd (119 ms on 32 cores against 649 ms
    # on 8, profiles/r02a_cpu_baseline_reference_container.json) — `value` is the port's rate, these are the reference's times.
    ref_live = ref if (isinstance(ref, dict) and "fwd_ms" in ref) else None
    ref_const = {"fwd_ms": 136.92, "bwd_ms": 648.66, "cores": 8} if workload_name == "S-1080p-1M" else None
    ref_short = ref_live or ref_const
    return {
        "value": 1.0 / total, "unit": "images/s", "cores": cores, "kind": "port", "reference_projection_sh": ref,
        "ref_fwd_ms": ref_short["fwd_ms"] if ref_short else None, "ref_bwd_ms": ref_short["bwd_ms"] if ref_short else None,
        "ref_cores": ref_short["cores"] if ref_short else None,
        "ref_source": ("measured in this run (reference tree present)" if ref_live else
                       ("constant: 8-vCPU build container, profiles/r02a_cpu_baseline_reference_container.json" if ref_const else None)),
        "kind_note": "port = the oracle's restatement, NOT the reference's code: its projection + SH backward runs ~5 x faster than the reference's own "
                     "autograd (ref_* keys: the reference's project_gaussians + eval_sh forward / backward, north_star's CPU baseline)",
        # The number north_star names — the reference's OWN project_gaussians + eval_sh on host cores — cannot be measured on the GPU
        # box (no reference tree there: `reference_projection_sh` is null in the driver's line).  What was measured where the tree
        # exists, as a labelled CONSTANT beside the live port figure: the 8-vCPU build container, S-1080p-1M,
        # profiles/r02a_cpu_baseline_reference_container.json.
        "reference_projection_sh_build_container": (
            {"kind": "reference", "fwd_ms": 136.92, "bwd_ms": 648.66, "cores": 8, "workload": "S-1080p-1M", "measured": "constant, not this run",
             "source": "profiles/r02a_cpu_baseline_reference_container.json"} if workload_name == "S-1080p-1M" else None),
        "value_with_numpy_binning": 1.0 / (total + binning_s),
        "binning_note": "ms.binning is the oracle's numpy restatement of the (tile | depth) key sort — test infrastructure, not a baseline; excluded from value",
        "sample": f"one fwd+bwd pass of {workload_name} (N={wl['n']}, {W}x{H}, I={int(flat.shape[0])}), fp32, "
                  f"torch CPU projection+SH (restating the reference's gaussian_projection.py/sh_utils.py) + OpenMP C compositing",
        "ms": {"project_sh_fwd": (t1 - t0) * 1e3, "binning": (t2 - t1) * 1e3, "composite_fwd": (t3 - t2) * 1e3,
               "composite_bwd": (t4 - t3) * 1e3, "project_sh_bwd": (t5 - t4) * 1e3},
    }


def reference_projection_sh(workload_name, cores):
    """The reference's OWN CPU/PyTorch path named by BASELINE.json (internal/utils/gaussian_projection.py:6-138
    project_gaussians + internal/utils/sh_utils.py:57-113 eval_sh), forward and autograd backward, timed on the host cores.
    Needs the reference tree (GSPL_REFERENCE_ROOT, default /root/reference): absent on the GPU boxes -> None."""
    import importlib.util
    from gspl_amd import synthetic
    root = os.environ.get("GSPL_REFERENCE_ROOT", "/root/reference")
    files = [os.path.join(root, "internal", "utils", f) for f in ("gaussian_projection.py", "sh_utils.py")]
    if not all(os.path.exists(f) for f in files):
        return None
    mods = []
    for i, f in enumerate(files):
        spec = importlib.util.spec_from_file_location(f"_gspl_ref_mod{i}", f)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods.append(m)
    gp, sh = mods
    wl = synthetic.WORKLOADS[workload_name]
    torch.set_num_threads(cores)
    means, scales, quats, opac, shs = synthetic.workload_scene(wl, seed=42)
    cam = synthetic.camera(wl["width"], wl["height"], wl["fx"])
    W, H = wl["width"], wl["height"]
    t = torch.tensor

    def one_pass():
        m, s, q, c = [x.clone().requires_grad_(True) for x in (means, scales, quats, shs)]
        t0 = time.perf_counter()
        res = gp.project_gaussians(means_3d=m, scales=s, scale_modifier=1.0, quaternions=q, world_to_camera=cam["world_to_camera"],
                                   fx=t(cam["fx"]), fy=t(cam["fy"]), cx=t(cam["cx"]), cy=t(cam["cy"]),
                                   img_height=t(H), img_width=t(W), block_width=16)
        xys, depths, radii, conics, comp = res[:5]
        dirs = m.detach() - cam["camera_center"]
        dirs = dirs / dirs.norm(dim=-1, keepdim=True)
        rgbs = torch.clamp_min(sh.eval_sh(3, c.transpose(1, 2), dirs) + 0.5, 0.0)      # [N,3,K] as vanilla_renderer.py:100
        t1 = time.perf_counter()
        (xys.sum() + conics.sum() + comp.sum() + rgbs.sum()).backward()
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3

    one_pass()                                   # warm-up
    runs = [one_pass() for _ in range(3)]
    fwd, bwd = min(r[0] for r in runs), min(r[1] for r in runs)
    return {"kind": "reference", "fwd_ms": round(fwd, 2), "bwd_ms": round(bwd, 2), "cores": cores, "root": root,
            "sample": f"{workload_name}: reference project_gaussians + eval_sh (degree 3), fp32, 1 warm-up + min of 3, sum() losses"}


def kernel_source_sha16():
    """Fingerprint of the compositing kernels' sources: a stored PMC traffic figure is only valid for the code it was measured on."""
    import hashlib
    h = hashlib.sha256()
    for f in ("composite_bwd.hip", "composite.hip", "gspl_composite.h"):
        with open(os.path.join(ROOT, "gaussian-splatting-lightning_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def pmc_traffic(workload_key, kernel):
    """(HBM bytes per launch, where the figure comes from) for the graded kernel, from the newest profiles/*_pmc_traffic.json whose
    recorded ABI version, kernel name and kernel-source fingerprint match what is loaded NOW (tools/make_pmc_traffic.py writes them;
    counters cannot be collected inside this run — rocprofv3 PMC passes are separate runs).  Anything else is refused: (None, why)."""
    from gspl_amd import _lib
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")), reverse=True)
    why = "no profiles/*_pmc_traffic.json"
    for path in files:
        name = os.path.basename(path)
        try:
            with open(path) as f:
                doc = json.load(f)
        except (OSError, ValueError) as e:
            why = f"{name}: unreadable ({e})"
            continue
        entry = (doc.get(workload_key) or {}).get(kernel) or {}
        if not entry.get("traffic_bytes"):
            why = f"{name}: no entry for {workload_key} / {kernel}"
            continue
        meta = doc.get("_measured_on") or {}
        if meta.get("abi_version") != _lib.ABI_VERSION or meta.get("kernel_source_sha16") != kernel_source_sha16():
            why = (f"{name} REFUSED: measured on ABI {meta.get('abi_version')} / sources {meta.get('kernel_source_sha16')}, "
                   f"loaded ABI {_lib.ABI_VERSION} / sources {kernel_source_sha16()}")
            continue
        return entry["traffic_bytes"], f"profiles/{name} ({entry.get('source', 'PMC passes')}; same ABI and kernel sources as this run)"
    return None, why


def main():
    args = parse()
    if args.api is None:      # the workload's API (configs[4] proxy: gsplat), vanilla otherwise — the reference's default renderer
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import gspl_amd  # noqa: F401
        from gspl_amd import synthetic as _syn
        args.api = _syn.WORKLOADS[args.workload].get("api", "vanilla")
    if args.cpu_baseline_only:
        sample = args.workload if args.cpu_sample == "auto" else args.cpu_sample
        print(json.dumps(cpu_baseline(sample, args.api)), flush=True)
        return
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            sys.exit("launch with: python -m torch.distributed.run --nnodes=1 --nproc-per-node N bench.py --gpus N ...")
    assert torch.cuda.is_available(), "bench.py needs a GPU (the HIP extension is the only compute path)"
    if args.share_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1 or args.init_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(args.dist_backend, rank=rank, world_size=world)
    mode = args.parallelism
    if mode == "auto":
        mode = "single" if world == 1 else "sharded"
    if mode == "single" and world > 1:
        sys.exit("--parallelism single needs --gpus 1")

    import gspl_amd  # noqa: F401
    from gspl_amd import _lib, ops, synthetic
    from gspl_amd import distributed as gdist
    from gspl_amd.density import update_densification_stats, update_densification_stats_views
    _lib.lib()
    if args.init_dist:
        gdist.SINGLE_RANK_SHORTCUT = False
    wl = synthetic.WORKLOADS[args.workload]
    W, H = wl["width"], wl["height"]
    means, scales, quats, opac, shs = synthetic.workload_scene(wl, seed=42)
    SH_DEGREE = wl.get("sh_degree", 3)
    # The camera set the steps cycle through: rank r takes camera (k * world + r) mod n at its step k (cameras sharded over the
    # ranks, one per rank per step).  Camera 0 is the pose the workload is defined on.
    n_cams = max(args.cameras, world)
    cam_dicts = synthetic.camera_set(W, H, wl["fx"], count=n_cams, distance=wl.get("distance", 4.0), kind=args.cameras_set)
    # the order the views are served in: a fresh random permutation per epoch (the reference's loader) for the heterogeneous set,
    # set order for the orbit set (rounds 3-5); the same on every rank
    view_stream = synthetic.ViewStream(n_cams, shuffled=(args.cameras_set == "heterogeneous"), seed=42)
    # eps 1e-15 as the reference (internal/models/vanilla_gaussian.py:266-300).  The bench tensors are ACTIVATED values
    # (post-exp scales, post-sigmoid opacities), so the reference's learning rates — meant for the raw parameters —
    # are scaled down by 1e3: the optimizer's cost is measured without letting the synthetic scene drift.
    LRS = (1.6e-4, 5e-3, 1e-3, 5e-2, 2.5e-3)         # means, scales, rotations, opacities, SH

    def make_optimizer(kind, groups):
        if kind == "none":
            return None
        if kind == "torch-adam":
            return torch.optim.Adam(groups, eps=1e-15)
        if kind == "masked-adam":
            if mode != "replicated":
                sys.exit("--optimizer masked-adam belongs to --parallelism replicated")
            return gdist.MaskedReplicaAdam([(str(i), g["params"][0], g["lr"]) for i, g in enumerate(groups)], eps=1e-15)
        from gspl_amd import optimizers as gopt
        # single GPU: the update of shs_rest (45 of a Gaussian's 59 floats) runs on the rasterizer's colour stream, under the next
        # frame's geometry and binning kernels (FusedAdam(deferred=...): same kernel, bit-identical parameters)
        deferred = ("shs_rest",) if (mode == "single" and args.overlap_sh_update and not args.no_overlap_sh_update) else None
        if kind == "fused-bwd-adam":
            # the same update applied by the rasterizer's backward (FusedAdam(fuse_into_backward=True), gspl_rasterize_inria_bwd_adam): the
            # parameter gradients never reach HBM.  Off until the step that has a `step()` behind every backward is built (below).
            if mode != "single" or api != "vanilla":
                sys.exit("--optimizer fused-bwd-adam: one GPU, vanilla API (the fused Inria backward applies the update)")
            opt = gopt.FusedAdam(groups, eps=1e-15, fuse_into_backward=True)
            opt.fuse_into_backward = False
            return opt
        return (gopt.FusedAdam if kind == "fused-adam" else gopt.SelectiveAdam)(groups, eps=1e-15, deferred=deferred)

    DENSIFY_INTERVAL = 100      # the reference consumes the statistics every 100 steps (vanilla_density_controller.py:16,86)
    counter = {"n": 0}
    transport_note = None

    if mode == "sharded":
        # ---- the reference's configs/distributed.yaml: Gaussians sharded, one packed all-to-all per step ------------------
        from gspl_amd.renderers import HipGSplatDistributedRenderer
        lo, hi = gdist.shard_bounds(wl["n"], world, rank)
        model = synthetic.ModelObject(*[t[lo:hi].contiguous().to(dev) for t in (means, scales, quats, opac, shs)])
        N = hi - lo
        cams = [synthetic.CameraObject(c, dev, idx=i) for i, c in enumerate(cam_dicts)]
        # tile_based_culling as in the reference's configs/distributed-accel.yaml (lossless here: same images and gradients)
        def make_renderer(transport):
            r = HipGSplatDistributedRenderer(tile_based_culling=True, fused_step=not args.staged_sharded_step,
                                             exchange=("auto" if (transport == "peer" and args.exchange == "counted") else args.exchange),
                                             exchange_transport=transport).instantiate()
            r.world_size, r.global_rank = world, rank
            r.camera_lookup = lambda idx, training: cams[idx]
            r.train()
            return r
        bg = torch.zeros(3, device=dev)
        transport, transport_note = args.exchange_transport, None
        if transport == "auto":
            transport = "collective"
            if world > 1 and not args.staged_sharded_step:
                # one validation frame over each transport: the forward is deterministic, so the peer route must reproduce the
                # collective route's image bit for bit on EVERY rank; a set-up failure or a mismatch anywhere keeps the collective
                ok, why = 1, "validated: one frame over the peer transport equals the collective route's image bit for bit on every rank"
                # the validation frame waits ~5 s for a peer's records, not a collective's patience (120 s by default): between GPUs whose
                # writes never become visible to each other it must cost seconds before the collective route is kept (the class
                # attribute is what every wait reads: the timed steps have the full budget again; GSPL_PEER_MAX_POLLS set = left alone)
                full_budget = gdist.PeerExchange.MAX_POLLS
                if "GSPL_PEER_MAX_POLLS" not in os.environ:
                    gdist.PeerExchange.MAX_POLLS = min(full_budget, 5_000_000)
                try:
                    ref_img = make_renderer("collective")(cams[rank % len(cams)], model, bg)["render"].detach()
                    candidate = make_renderer("peer")
                    img = candidate(cams[rank % len(cams)], model, bg)["render"].detach()
                    torch.cuda.synchronize()             # a wait that gave up has raised its error word by now
                    if candidate._peer is not None:
                        candidate._peer.check()
                    if candidate._peer is None or not torch.equal(img, ref_img):
                        ok, why = 0, "the peer route's validation frame differed from the collective route's (or the route was not taken)"
                except Exception as e:      # IPC mapping refused, shared memory unavailable, a peer's records never arrived, ...
                    ok, why = 0, f"peer transport set-up failed on rank {rank}: {e!r}"
                finally:
                    gdist.PeerExchange.MAX_POLLS = full_budget
                flag = torch.tensor([ok], device=dev, dtype=torch.int32)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                if int(flag.item()) == 1:
                    transport = "peer"
                elif ok == 1:
                    why = "another rank could not use the peer transport"
                transport_note = why
        renderer = candidate if (transport == "peer" and args.exchange_transport == "auto") else make_renderer(transport)
        args.exchange_transport = transport
        target = torch.full((3, H, W), 0.5, device=dev)
        loss_fn = (lambda img: ops.photometric_loss(img, target, 0.2)) if args.loss == "photometric" else (lambda img: (img - target).abs().mean())
        tensors = model.leaves()
        lrs = LRS[:4] + (LRS[4], LRS[4] / 20.0)
        grad_scale = torch.tensor([0.5 * W, 0.5 * H], device=dev)
        state = {}

        def step():
            for t in tensors:
                t.grad = None
            mine = cams[view_stream.view(state.setdefault("k", 0) * world + rank)]
            state["k"] += 1
            marks = state.get("marks")
            if marks is not None:
                marks.append(_mark())
            out = renderer(mine, model, bg)
            for r in out["projection_results_list"]:      # DistributedVanillaDensityControllerImpl.before_backward
                r[1].retain_grad()
            loss = loss_fn(out["render"])
            if marks is not None:
                marks.append(_mark())
            loss.backward()
            if marks is not None:
                marks.append(_mark())
            state["out"], state["loss"] = out, loss
            return state
        step.state = state

        def stats(st, accum, denom, max_radii):           # DistributedVanillaDensityControllerImpl.update_states: every camera of the step, one launch
            out = st["out"]
            update_densification_stats_views([r[1].grad for r in out["projection_results_list"]], out["visible_mask_list"],
                                             [r[0] for r in out["projection_results_list"]], accum, denom, max_radii, scale=grad_scale)
        visible = None
        api = "gsplat"
    else:
        # the reference model's parameters: the SH coefficients are two of them, shs_dc [N,1,3] and shs_rest [N,15,3]
        tensors = [t.contiguous().to(dev).requires_grad_(True) for t in (means, scales, quats, opac, shs[:, :1], shs[:, 1:]) if t.shape[1] > 0]
        N = wl["n"]
        step = make_step(args.api, dev, wl, cam_dicts, tensors, args.loss, rank, world, stream=view_stream)
        lrs = (LRS[:4] + (LRS[4], LRS[4] / 20.0))[:len(tensors)]

        def stats(st, accum, denom, max_radii):
            densification_stats(st, accum, denom, max_radii)
        api = args.api

    accum = torch.zeros(N, device=dev)
    denom = torch.zeros(N, device=dev)
    max_radii = torch.zeros(N, device=dev)                       # float, as the reference's buffer (vanilla_density_controller.py:61)
    if mode != "sharded" and api == "vanilla":
        step.state["stats_buffers"] = (accum, denom, max_radii)

    def make_full_step(optimizer, opt_kind):
        def full_step(force_reduce=False):
            if opt_kind == "fused-bwd-adam":
                optimizer.fuse_into_backward = True       # (a plain attribute store; the other passes of the bench run with it off)
            st = step()
            if opt_kind == "fused-bwd-adam":
                optimizer.fuse_into_backward = False
            with torch.no_grad():
                stats(st, accum, denom, max_radii)
                if optimizer is not None:
                    if opt_kind == "masked-adam":
                        # replicas stay identical: rows ANY rank saw are reduce-scattered to their owners, updated there and
                        # all-gathered back (distributed.MaskedReplicaAdam)
                        optimizer.step(st["radii"] > 0)
                        counter["n"] += 1
                        if force_reduce or counter["n"] % DENSIFY_INTERVAL == 0:
                            gdist.reduce_densification_stats(accum, denom, max_radii)
                        return st
                    if mode == "replicated" and opt_kind == "fused-adam":
                        # replicas stay identical: the parameter gradients are averaged over the ranks (DDP of configs/ddp.yaml) in
                        # chunks, and every chunk is updated by the fused Adam while the next ones are still being reduced
                        gdist.all_reduce_and_step(optimizer, tensors)
                        counter["n"] += 1
                        if force_reduce or counter["n"] % DENSIFY_INTERVAL == 0:
                            gdist.reduce_densification_stats(accum, denom, max_radii)
                        return st
                    if mode == "replicated":
                        gdist.all_reduce_gradients(tensors)
                    if opt_kind == "selective-adam" and "radii" in st:
                        optimizer.step(st["radii"] > 0)
                    else:
                        optimizer.step()
                counter["n"] += 1
                # replicated mode: the statistics are accumulated locally and made identical on all ranks when a densification
                # would consume them (every DENSIFY_INTERVAL steps) — and once at the end of the timed region so that every
                # run pays for at least one reduction.  Sharded mode: every rank keeps the statistics of its own rows.
                if mode == "replicated" and (force_reduce or counter["n"] % DENSIFY_INTERVAL == 0):
                    gdist.reduce_densification_stats(accum, denom, max_radii)
            return st
        return full_step

    PROFILE_PERIOD = 1 if args.stage_times else 4

    def timed_region(full_step, steps, warmup, instrumented=False):
        # instrumented=False — the contract's timed region: NO per-step events (an event record idles the stream for ~6-7 us:
        # profiles/r05d_sequence.txt, the three gaps at the step's marks; three per step were 1.6 % of the step); only the GRADED
        # kernel's launch is bracketed, every fourth step, for `roofline` ("HIP events over the timed region").
        # instrumented=True — the pass that follows it, same steps: three events per step (fwd_ms / bwd_ms / step_ms percentiles)
        # and the forward compositing launch bracketed too.
        # Host hygiene: a full (generation-2) pass of Python's cyclic GC walks every object torch has imported — 30-40 ms during
        # which no kernel is launched, once every ~130 steps.  Freezing what exists once the first warm-up steps have created their
        # lazily-built objects keeps later collections to the objects of the steps themselves.  The collection sits INSIDE the
        # warm-up (before its last steps), not between warm-up and timed region, and it is the SECOND one of the process (the first,
        # before the per-camera pass, froze the imported world): with the driver's five warm-up steps a 35 ms walk three steps ahead
        # of the timed region cost it 1.8 % (profiles/r11a_warmup_length.txt: 1.287 ms per step with 5 warm-up steps, 1.263 with 50,
        # the per-step percentiles of the pass that follows identical) — tens of milliseconds of idle device right before the timed
        # steps is what a training loop never has.
        early = min(warmup, 2) if os.environ.get("GSPL_BENCH_GC_LATE") is None else warmup
        for _ in range(int(os.environ.get("GSPL_BENCH_PREHEAT", "0"))):      # diagnostic: extra untimed steps ahead of the warm-up
            full_step(force_reduce=True)
        for _ in range(early):
            full_step(force_reduce=True)
        gc.collect()
        gc.freeze()
        for _ in range(warmup - early):
            full_step(force_reduce=True)
        if dist is not None:
            dist.barrier()
            # RCCL writes its version banner through C stdio, which on a pipe would come out at exit, AFTER the JSON line:
            # push it out now, so that the line rank 0 prints stays the last line of stdout
            import ctypes
            ctypes.CDLL(None).fflush(None)
        torch.cuda.synchronize()
        if instrumented:
            step.state["marks"] = []
        else:
            step.state.pop("marks", None)
        ops.SPECULATION.update(frames=0, cold=0, misses=0)
        # the roofline needs the launch duration of the graded kernel from HIP events on its stream; an event pair idles the stream
        # for ~6 us on either side of the launch, so only every fourth launch is bracketed
        graded = ("gspl_composite_bwd_packed", "gspl_composite_bwd")
        _lib.profile_start(None if (args.stage_times and instrumented) else (graded + ("gspl_composite_fwd",) if instrumented else graded),
                           period=PROFILE_PERIOD if instrumented else 4)
        mallocs0 = torch.cuda.memory_stats(dev).get("num_device_alloc", 0)
        t0 = time.perf_counter()
        for k in range(steps):
            full_step(force_reduce=(k == steps - 1))
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        # hipMalloc calls of torch's caching allocator inside the timed region (a new list capacity that no cached block holds)
        step.state["device_mallocs"] = torch.cuda.memory_stats(dev).get("num_device_alloc", 0) - mallocs0
        prof = _lib.profile_stop()
        marks = step.state.pop("marks", [])
        if dist is not None:
            t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        return elapsed, prof, marks

    GROUP_NAMES = ("means", "scales", "rotations", "opacities", "shs_dc", "shs_rest")
    if os.environ.get("GSPL_BENCH_RESERVE_GB"):
        _r = torch.empty(int(float(os.environ["GSPL_BENCH_RESERVE_GB"]) * (1 << 30)), dtype=torch.uint8, device=dev)
        del _r
    groups = [{"params": [t], "lr": lr * 1e-3, "name": n} for t, lr, n in zip(tensors, lrs, GROUP_NAMES)]
    optimizer = make_optimizer(args.optimizer, groups)
    # ---- per-camera pass BEFORE the warm-up (one forward + backward per camera of the set, no parameter update) ------------------
    # It produces the workload the byte / flop models are evaluated on (I, I', V and the blended pairs of every camera, below) and
    # it is the first pass over the data set: when the contract's W warm-up steps start, the allocator holds blocks for every
    # camera's list sizes and the device is at its clocks — the state of a training run past its first epoch, which is what
    # `value` is about.  (Measured with the driver's `--steps 20 --warmup 5`: 1.306-1.313 ms per step straight after start-up — three
    # hipMallocs inside the timed region — against 1.26-1.29 ms after 21 or more warm-up steps; profiles/r04e.)
    # Host hygiene, part 1 (see timed_region): the one expensive walk of Python's cyclic GC over everything torch has imported
    # (30-40 ms) happens HERE, a whole pass over the camera set away from the timed steps; the collection inside the warm-up then
    # only sees the objects the first steps created (well under a millisecond) and leaves the device no time to drop its clocks.
    import gc
    if os.environ.get("GSPL_BENCH_GC_EARLY", "1") != "0":      # "0": diagnostic, the one walk inside the warm-up as before
        gc.collect()
        gc.freeze()
    ops.KEEP_LAST_RASTER = True
    per_cam_before = []
    if mode != "sharded" and not args.no_workload_stats:
        with torch.no_grad():
            probe = make_step(api, dev, wl, cam_dicts, tensors, args.loss, 0, 1)
            for i, c0 in enumerate(cam_dicts):
                with torch.enable_grad():
                    probe()                                   # one step on camera i: leaves its projected splats and lists in LAST_RASTER
                last = ops.LAST_RASTER
                count = ops.composite_scores(last["means2d"], last["conics"], last["opacities"], W, H, 16, last["offsets"],
                                             last["flatten_ids"], mode=last["mode"])[0]
                entry = {"list_entries": int(last["flatten_ids"].shape[0]), "valid_pairs": int(count.sum(dtype=torch.int64).item()),
                         "entries_walked": entries_walked(last, W, H)}
                if api == "vanilla":      # every tile-rect intersection in the Inria convention: the same binning without culling
                    entry["I"] = int(ops.bin_gaussians(last["means2d"], last["depths"], last["radii"], H, W, 16, mode=_lib.GSPL_MODE_INRIA)[0].shape[0])
                    entry["V"] = int((last["radii"] > 0).sum().item())
                else:
                    m, s_, q = tensors[:3]
                    vm = c0["world_to_camera"].T.contiguous().to(dev)
                    pr = ops.project_gaussians(m, s_, 1.0, q, vm[:3], c0["fx"], c0["fy"], c0["cx"], c0["cy"], H, W, 16)
                    entry["I"], entry["V"] = int(pr[5].sum().item()), int((pr[2] > 0).sum().item())
                per_cam_before.append(entry)
            for t in tensors:
                t.grad = None
    elif mode == "sharded" and not args.no_workload_stats:
        # the sharded step's first pass over the camera set (every rank takes its cameras: the collectives pair up); its statistics
        # are taken after the timed region, from the projection of every camera and rank 0's last frame
        for _ in range((len(cam_dicts) + world - 1) // world):
            step()
        step.state["k"] = 0
        for t in tensors:
            t.grad = None
    ops.LAST_RASTER = None
    the_step = make_full_step(optimizer, args.optimizer)
    if args.dump_outputs:
        step.state["keep_render"] = True
    elapsed, prof_graded, _ = timed_region(the_step, args.steps, args.warmup)
    dumped = None
    if args.dump_outputs:
        step.state.pop("keep_render")
        if rank == 0:
            dumped = dump_outputs(args.dump_outputs, step.state, list(zip(GROUP_NAMES, tensors)),
                                  [("grad_accum", accum), ("denom", denom), ("max_radii", max_radii)], counter["n"])
        step.state.pop("render", None)
    device_mallocs = step.state.get("device_mallocs")
    speculation = dict(ops.SPECULATION)
    # the instrumented pass: the same steps again, with the per-step events
    elapsed_instrumented, prof, marks = timed_region(the_step, args.steps, 0, instrumented=True)
    for k_, v_ in prof_graded.items():          # the graded kernel's durations are the timed region's
        prof[k_] = v_
    phase_fwd = sum(marks[i].elapsed_time(marks[i + 1]) for i in range(0, len(marks), 3)) / args.steps
    phase_bwd = sum(marks[i + 1].elapsed_time(marks[i + 2]) for i in range(0, len(marks), 3)) / args.steps
    # device-side span of every step of the timed region: start of step i to start of step i + 1
    starts = marks[0::3]
    spans = sorted(starts[i].elapsed_time(starts[i + 1]) for i in range(len(starts) - 1))
    pct = (lambda q: round(spans[min(len(spans) - 1, int(q * len(spans)))], 4)) if spans else (lambda q: None)
    step_ms = {"p50": pct(0.50), "p90": pct(0.90), "p99": pct(0.99), "max": round(spans[-1], 4) if spans else None}
    raw_spans = [starts[i].elapsed_time(starts[i + 1]) for i in range(len(starts) - 1)]
    step_ms["slowest"] = [[i, round(v, 3)] for v, i in sorted(((v, i) for i, v in enumerate(raw_spans)), reverse=True)[:3]]
    if os.environ.get("GSPL_BENCH_DUMP_STEPS"):
        print("step spans (ms):", " ".join(f"{v:.3f}" for v in raw_spans), file=sys.stderr)
    renderer_only = None
    if world == 1 and optimizer is not None and not args.no_renderer_only:
        # second timed region of the same run: the step without a parameter update (round 1's `value`)
        e2, _, m2 = timed_region(make_full_step(None, "none"), args.steps, 2, instrumented=True)
        renderer_only = {"images_per_s": round(args.steps / e2, 3), "ms_per_step": round(e2 / args.steps * 1e3, 4),
                         "fwd_ms": round(sum(m2[i].elapsed_time(m2[i + 1]) for i in range(0, len(m2), 3)) / args.steps, 4),
                         "bwd_ms": round(sum(m2[i + 1].elapsed_time(m2[i + 2]) for i in range(0, len(m2), 3)) / args.steps, 4)}

    # third timed region of the same run: the same step with the optimizer INSIDE the backward (FusedAdam(fuse_into_backward=True),
    # gspl_rasterize_inria_bwd_adam) — opt-in in the product, so it is not `value`; reported beside it
    fused_bwd_adam = None
    if world == 1 and mode == "single" and api == "vanilla" and args.optimizer == "fused-adam" and not args.no_renderer_only:
        try:
            opt2 = make_optimizer("fused-bwd-adam", [{"params": [t], "lr": lr * 1e-3, "name": n} for t, lr, n in zip(tensors, lrs, GROUP_NAMES)])
            e3, _, _ = timed_region(make_full_step(opt2, "fused-bwd-adam"), args.steps, 3)
            fused_bwd_adam = {"images_per_s": round(args.steps / e3, 3), "ms_per_step": round(e3 / args.steps * 1e3, 4),
                              "what": "optimizer = FusedAdam(fuse_into_backward=True): the per-Gaussian kernels that end the backward apply the Adam "
                                      "update (no parameter gradient in HBM); bit-identical parameters, opt-in (tests/test_fused_backward_adam.py)"}
            del opt2
        except Exception as e:      # an extra: it must never take the bench line down
            fused_bwd_adam = {"failed": repr(e)}

    # ---- the workload the byte / flop models are evaluated on: per camera of the set, averaged --------------------------------
    # I = every tile-rect intersection of the API benched, I' = list entries the kernels walk after the lossless
    # tile culling, V = visible splats, valid pairs = (pixel, splat) pairs the compositing blends (COUNTED on the device).
    per_cam = []
    with torch.no_grad():
        if args.no_workload_stats:
            pass
        elif mode == "sharded":
            m, s_, q = tensors[0], tensors[1], tensors[2]
            for c0 in cam_dicts:
                vm = c0["world_to_camera"].T.contiguous().to(dev)
                pr = ops.project_gaussians(m, s_, 1.0, q, vm[:3], c0["fx"], c0["fy"], c0["cx"], c0["cy"], H, W, 16)
                cnt = torch.stack([pr[5].sum(dtype=torch.int64), (pr[2] > 0).sum(dtype=torch.int64)])
                if dist is not None:
                    dist.all_reduce(cnt, op=dist.ReduceOp.SUM)
                per_cam.append({"I": int(cnt[0].item()), "V": int(cnt[1].item())})
            if rank == 0 and ops.LAST_RASTER is not None:      # lists and blended pairs of rank 0's last frame (its own camera)
                last = ops.LAST_RASTER
                count = ops.composite_scores(last["means2d"], last["conics"], last["opacities"], W, H, 16, last["offsets"],
                                             last["flatten_ids"], mode=last["mode"])[0]
                for e in per_cam:
                    e["list_entries"], e["valid_pairs"] = int(last["flatten_ids"].shape[0]), int(count.sum(dtype=torch.int64).item())
                    if last.get("last_ids") is not None:
                        e["entries_walked"] = entries_walked(last, W, H)
        else:
            per_cam = per_cam_before

    # ---- stage rooflines: a STAGED pass (one C-ABI call per stage instead of the fused calls) with an event pair around every call,
    # after the timed regions; the SH kernel once overlapped with the binning on its side stream (as in the step) and once alone.
    stage_prof = None
    if rank == 0 and mode == "single" and api == "vanilla" and not args.no_stage_rooflines:
        def staged_pass(side_stream):
            os.environ["GSPL_SIDE_STREAM"] = "1" if side_stream else "0"
            fused, ops.FUSED_INRIA = ops.FUSED_INRIA, False
            try:
                fs = make_full_step(optimizer, args.optimizer)
                for _ in range(3):
                    fs()
                torch.cuda.synchronize()
                _lib.profile_start(None, period=1)
                for _ in range(len(cam_dicts)):
                    fs()
                return _lib.profile_stop()
            finally:
                ops.FUSED_INRIA = fused
                os.environ.pop("GSPL_SIDE_STREAM", None)
        stage_prof = {"overlapped": staged_pass(True), "alone": staged_pass(False)}

    if rank == 0:
        mean = lambda name: (sum(prof[name]) / len(prof[name])) if prof.get(name) else None
        # per-STEP totals (an entry point called twice per step, e.g. the two phases of the Inria preprocess, counts twice)
        # (with sampled timing: mean of the timed calls x calls per step)
        period_of = lambda k: 4 if (k in prof_graded) else PROFILE_PERIOD
        stages = {k: round(sum(v) / len(v) * max(1, round(len(v) * period_of(k) / args.steps)), 4) for k, v in prof.items() if v}
        P = W * H
        bwd_ms = mean("gspl_composite_bwd_packed") or mean("gspl_composite_bwd")
        avg = lambda key: (sum(e[key] for e in per_cam) / len(per_cam)) if per_cam and key in per_cam[0] else None
        I, list_entries, valid_pairs, V = avg("I"), avg("list_entries"), avg("valid_pairs"), avg("V")
        walked = avg("entries_walked")
        roofline = None
        if bwd_ms and per_cam:
            kernel = _lib.lib().gspl_composite_bwd_kernel_name().decode()
            traffic, traffic_source = pmc_traffic(f"{args.workload}/{api}", kernel)
            t_s = bwd_ms * 1e-3
            bytes_I = (76.0 * I + 20.0 * P) if I is not None else None
            bytes_L = (76.0 * list_entries + 20.0 * P) if list_entries is not None else None
            bytes_W = (76.0 * walked + 20.0 * P) if walked is not None else None
            # The launch walks the CULLED per-tile lists (I') from each tile's deepest blended entry to its head, so `frac` is priced on
            # the entries WALKED (round 5: in a saturating scene the lists continue far behind the stop and the kernel never reads that
            # part; at the metric point walked ~ I').  The figures on I' (rounds 4) and on every rect intersection of the benched API
            # (I: what SURVEY.md §8(d) counts and rounds 1-3 reported as `frac`) stay beside it.
            alg = bytes_W if bytes_W is not None else (bytes_L if bytes_L is not None else bytes_I)
            achieved = alg / t_s / 1e9
            roofline = {"bound": "hbm", "kernel": kernel, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic, "traffic_source": traffic_source,
                        "algorithmic_bytes": alg, "bytes_model": "76 B x list entries the launch walks + 20 B x pixels",
                        "avg_ms": round(bwd_ms, 4),
                        "intersections": I, "list_entries": list_entries, "entries_walked": walked,
                        "frac_on_list_entries": round(bytes_L / t_s / 1e9 / HBM_PEAK_GBS, 5) if bytes_L else None,
                        "frac_on_rect_intersections": round(bytes_I / t_s / 1e9 / HBM_PEAK_GBS, 5) if bytes_I else None,
                        "valid_pairs": valid_pairs, "flop_per_pair": 70,
                        "valu_frac": round(valid_pairs * 70.0 / t_s / (FP32_PEAK_TFLOPS * 1e12), 5) if valid_pairs else None,
                        "valu_peak_tflops": FP32_PEAK_TFLOPS,
                        "workload_mean_over_cameras": len(per_cam)}
        # ---- every stage of the step against the HBM roofline: SURVEY.md §8(d) bytes / measured duration / 8 TB/s ------------------
        stage_rooflines = None
        if stage_prof is not None and I is not None and V is not None:
            K = 16
            N_, Ip = float(wl["n"]), float(list_entries)
            Iw = float(walked) if walked is not None else Ip
            ov, al = stage_prof["overlapped"], stage_prof["alone"]
            per_step = lambda pr, names: (sum(sum(pr.get(n, [])) for n in names) / len(cam_dicts)) if any(pr.get(n) for n in names) else None
            phase = lambda pr, k: (lambda v: (sum(v[k::2]) / max(len(v[k::2]), 1)) if v else None)(pr.get("gspl_inria_preprocess_fwd", []))
            _frac_on = lambda ms, nbytes: round(nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if ms else None
            def entry(ms, nbytes, formula, **extra):
                if not ms:
                    return None
                gbs = nbytes / (ms * 1e-3) / 1e9
                return {"ms": round(ms, 4), "bytes": int(nbytes), "GBps": round(gbs, 1), "frac": round(gbs / HBM_PEAK_GBS, 4), "bytes_model": formula, **extra}
            bin_names = ("gspl_bin_count", "gspl_bin_emit", "gspl_bin_sort", "gspl_bin_sort_device_count", "gspl_bin_emit_sort")
            stage_rooflines = {
                "method": f"staged pass after the timed regions ({len(cam_dicts)} steps, one per camera): stage-by-stage C-ABI calls (GSPL_FUSED_INRIA=0) "
                          "with a HIP event pair around every call; bytes = SURVEY.md §8(d) per-unit figures x mean units over the camera set",
                "units": {"N": int(N_), "V": round(V, 1), "I": round(I, 1), "list_entries": round(Ip, 1), "entries_walked": round(Iw, 1), "P": P},
                "inria_preprocess_fwd": entry(phase(al, 0), 76.0 * N_, "76 N"),
                "sh_fwd_alone": entry(phase(al, 1), (12.0 * K + 24.0) * V, "(12 K + 24) V"),
                "sh_fwd_overlapped_with_binning": entry(phase(ov, 1), (12.0 * K + 24.0) * V, "(12 K + 24) V"),
                "binning": entry(per_step(al, bin_names), 72.0 * N_ + 32.0 * V + 44.0 * Ip,
                                 "depth sort 8 N (1 + 2*4) + emit 32 V + 8 I' + tile sort 36 I'"),
                "composite_fwd": entry(per_step(al, ("gspl_composite_fwd",)), 40.0 * Iw + 20.0 * P, "40 x entries walked + 20 P",
                                       frac_on_list_entries=_frac_on(per_step(al, ("gspl_composite_fwd",)), 40.0 * Ip + 20.0 * P),
                                       frac_on_rect_intersections=_frac_on(per_step(al, ("gspl_composite_fwd",)), 40.0 * I + 20.0 * P)),
                "composite_bwd": entry(per_step(al, ("gspl_composite_bwd_packed",)), 76.0 * Iw + 20.0 * P, "76 x entries walked + 20 P",
                                       frac_on_list_entries=_frac_on(per_step(al, ("gspl_composite_bwd_packed",)), 76.0 * Ip + 20.0 * P),
                                       frac_on_rect_intersections=_frac_on(per_step(al, ("gspl_composite_bwd_packed",)), 76.0 * I + 20.0 * P)),
                "inria_preprocess_bwd_with_sh_bwd": entry(per_step(al, ("gspl_inria_preprocess_bwd",)), (116.0 + 24.0 * K) * V, "(36 + 40 + 40) V + 2 * 12 K V"),
                "loss_fwd_bwd": entry(per_step(al, ("gspl_loss_l1_ssim_fwd", "gspl_loss_photometric_fwd", "gspl_loss_l1_ssim_bwd")), 4.0 * 3 * P * (2 + 3 + 4), "3 P floats: 2 read fwd, 3 maps written, 3 read + 1 written bwd"),
                "adam": entry(per_step(al, ("gspl_selective_adam", "gspl_selective_adam_limited")), 28.0 * 59.0 * N_, "28 B x 59 floats x N (param, grad, two moments read; param, two moments written)"),
                "densify_stats": entry(per_step(al, ("gspl_densify_stats",)), 29.0 * N_, "grad 12 + radii 4 + three buffers 12 read, up to 12 written, + mask 1"),
            }
        step_desc = ("renderer fwd + " + ("L1 loss" if args.loss == "l1" else "0.8 L1 + 0.2 (1-SSIM) loss (fused)") + " + full bwd"
                     + (" + gradient all-reduce" if mode == "replicated" and args.optimizer != "none" else "")
                     + ("" if args.optimizer == "none" else " + " + args.optimizer + " step")
                     + (" (shs_rest update on the colour stream, under the next frame's geometry + binning)"
                        if (mode == "single" and args.optimizer in ("fused-adam", "selective-adam") and args.overlap_sh_update and not args.no_overlap_sh_update) else "")
                     + " + densification stats")
        par = {"single": "single GPU",
               "replicated": (f"replicated Gaussians, {world} camera(s)/step, "
                              + ("visibility-masked reduce-scatter of the gradient rows to their owners + masked Adam on the owner + all-gather of the updated rows"
                                 if args.optimizer == "masked-adam" else
                                 "chunked all-reduce of the parameter gradients overlapped with the chunk-wise fused Adam every step")
                              + f", all-reduce of the densification stats every {DENSIFY_INTERVAL} steps"),
               "sharded": f"Gaussians sharded over {world} rank(s), {world} camera(s)/step, packed all-to-all of splat records (configs/distributed.yaml); "
                          + (f"exchange format of the last step: {renderer.last_exchange} over the {args.exchange_transport} transport"
                             + (f" ({transport_note})" if transport_note else "") + "; step as "
                             + ("eleven stage-by-stage autograd nodes" if args.staged_sharded_step else "three autograd nodes (front / exchange / back)")
                             if mode == "sharded" else "")}[mode]
        line = {
            "metric": "training images/sec + fwd/bwd ms @1080p, 1M Gaussians, 1/2/4/8 MI355X",
            "value": round(world * args.steps / elapsed, 3), "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": args.workload, "api": api, "n_gaussians": wl["n"], "width": W, "height": H,
                       "sh_degree": SH_DEGREE, "absgrad": bool(wl.get("absgrad", False)), "loss": args.loss, "optimizer": args.optimizer, "step": step_desc,
                       "parallelism": par, "parallelism_mode": mode,
                       **({"init_dist": f"process group of one rank on {args.dist_backend}: every collective of this mode is issued (code-path run, not a scaling point)"}
                          if args.init_dist else {})},
            "images_per_s_with_optimizer": round(world * args.steps / elapsed, 3) if args.optimizer != "none" else None,
            "images_per_s_renderer_only": (renderer_only["images_per_s"] if renderer_only else
                                           (round(world * args.steps / elapsed, 3) if args.optimizer == "none" else None)),
            "renderer_only": renderer_only,
            "with_fused_bwd_adam": fused_bwd_adam,
            "stages_ms": stages,
            # device time between the events at the start of the step, before loss.backward() and after it
            "fwd_ms": round(phase_fwd, 4),
            "bwd_ms": round(phase_bwd, 4),
            # fwd_ms / bwd_ms / step_ms / stages_ms.gspl_composite_fwd: from the instrumented pass right after the timed region (same
            # steps + three events per step, each a ~6-7 us idle stream); the timed region itself carries no per-step events, only
            # the graded kernel's launch is bracketed every fourth step (roofline.avg_ms)
            "instrumented_pass": {"ms_per_step": round(elapsed_instrumented / args.steps * 1e3, 4), "events_per_step": 3},
            "roofline": roofline,
            "stage_rooflines": stage_rooflines,
            # device-side span of a step (start to start) over the timed region
            "step_ms": step_ms,
            # list-length speculation of the binning (room = a decayed running maximum of the list entries per splat x N x 1.125 + 64 K,
            # ops._state.ListCapacity; a miss repeats emission, sort and compositing): frames of the timed region, frames without any
            # history, frames that needed more room than they were given
            "speculation": {**speculation, "miss_rate": round(speculation["misses"] / max(speculation["frames"], 1), 4)},
            "allocator": {"device_mallocs_in_timed_region": device_mallocs},
            "untimed_before_warmup": (None if args.no_workload_stats else
                                      "one forward + backward per camera of the set, no parameter update (the workload-statistics pass / first pass over the data set)"),
            "cameras": {"count": len(cam_dicts), "set": args.cameras_set,
                        "order": ("a fresh random permutation per epoch (synthetic.epoch_order, seed 42; internal/dataset.py:216-217)"
                                  if view_stream.shuffled else "set order, cyclically"),
                        "list_length_max_over_min": (round(max(e["list_entries"] for e in per_cam) / max(min(e["list_entries"] for e in per_cam), 1), 3)
                                                     if per_cam and "list_entries" in per_cam[0] else None),
                        "per_camera": per_cam if len(per_cam) <= 64 else None},
        }
        if dumped is not None:
            line["dumped_outputs"] = dumped
        if world == 1 and mode == "single" and args.loop == "reference-shaped" and api == "vanilla" and SH_DEGREE == 3:
            try:
                line["reference_shaped_loop"] = reference_shaped_loop(dev, wl, cam_dicts, args.loop_steps, prewarm=True, view_stream=view_stream)
                # the same loop with the activations left to torch (what the reference's renderer does with the same model)
                if not args.no_loop_comparison:
                    other = reference_shaped_loop(dev, wl, cam_dicts, args.loop_steps, fuse_activations=False, view_stream=view_stream)
                    line["reference_shaped_loop"]["with_torch_activations"] = {
                        k: other[k] for k in ("activations", "images_per_s_densifying", "ms_per_step_mean", "ms_per_step_between_events_p50", "n_end")}
                    # ... and with the optimizers' updates applied by the rasterizer's backward (opt-in; on a densification step the
                    # reference drops the step's gradients — the surgery replaces the Parameters before step() — here they were applied)
                    fused = reference_shaped_loop(dev, wl, cam_dicts, args.loop_steps, fuse_optimizer=True, view_stream=view_stream)
                    line["reference_shaped_loop"]["with_fused_bwd_adam"] = {
                        k: fused[k] for k in ("images_per_s_densifying", "ms_per_step_mean", "ms_per_step_between_events_p50", "n_end", "loss_first_last")}
                    # ... and once more with host-side counters read after every step (hipMallocs, cold / missed speculation): where the
                    # mean's excess over the quiet median goes; its own timing is not reported as a rate
                    traced = reference_shaped_loop(dev, wl, cam_dicts, args.loop_steps, view_stream=view_stream, per_step=True)
                    line["reference_shaped_loop"]["attribution"] = traced["attribution"]
            except Exception as e:  # an extra: it must never take the bench line down
                line["reference_shaped_loop"] = {"failed": repr(e)}
        if world == 1 and not args.no_cpu_baseline:
            sample = args.workload if args.cpu_sample == "auto" else args.cpu_sample
            try:
                line["cpu_baseline"] = cpu_baseline(sample, args.api)
            except Exception as e:  # the baseline leg must never take the bench line down
                line["cpu_baseline"] = {"value": None, "unit": "images/s", "cores": os.cpu_count(), "kind": "port",
                                        "sample": f"failed: {e!r}"}
        print(json.dumps(line), flush=True)
    if dist is not None:
        # Every rank is past its last collective and rank 0 has printed the line: leave without the collective tear-down and without
        # interpreter finalisation.  A worker of the eight-rank gloo tests was seen to die of SIGABRT in exactly that phase ("terminate
        # called without an active exception", after all results were in) — the launcher would report a failed run for a finished one.
        dist.barrier()
        if os.environ.get("GSPL_BENCH_SOFT_EXIT", "0") != "0":      # a profiler that writes its output when the process finalises
            dist.destroy_process_group()                             # (tools/profile_w8_shared_gpu.sh)
            return
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)


if __name__ == "__main__":
    main()

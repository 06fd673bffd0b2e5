"""The appearance MLP of the appearance-embedding route: `ops.appearance_mlp` (csrc/appearance.hip) against the reference's formulation
written with float32 torch ops — a boolean gather of the visible rows, `embedding.repeat`, a concat, three Linear layers, a boolean
scatter — on the same GPU, in one process, the two routes alternating repeat by repeat; and the plugin's whole step with the fused
network against the same plugin with `fused_mlp=False`.

(a) The default network (64 features + 32 embedding -> 64 -> 64 -> 3): N = 1 M with 30 % of the rows visible, N = 1 M with every row,
    N = 100 k with every row; and the view-dependent network (4 frequencies) at N = 1 M with 30 %.  Forward + backward, all gradients
    (features, weights, biases, embedding).  Per repeat the mean device time of `--steps` calls after `--warmup`; reported are the
    MINIMUM and the spread (max - min) over the repeats.  Peak memory above the inputs, per route.
    Bounds: the fused forward + backward needs FLOP_ROW floating-point operations per visible row (forward, the recomputed forward,
    the data gradients and the weight gradients: four passes over the layers) against the 157.3 TF fp32 matrix peak, and per row one
    read of the feature row, one write of its gradient row, the output row and its gradient against 8 TB/s.
    `worst_gradient_difference_over_max` compares the two float32 routes with each other: at 1 M rows a few pre-activations lie
    within an ulp of zero and take different sides of the ReLU in the two routes, which moves single `v_features` rows by percents
    of the tensor's maximum (either route differs from an fp64 evaluation by the same amount).
(b) One training step (forward, L1 loss, backward) of the plugin on S-800-100k after the warm-up, fused against the torch path.

The process ends itself after `--time-limit` seconds.
  python tools/appearance_mlp_time.py [--steps 10] [--warmup 3] [--repeats 5] [--out profiles/appearance_mlp_time.json]"""
import argparse
import json
import os
import signal
import types

import _step_time as T  # noqa: F401  (puts the repository root on sys.path)
import torch

PEAK_FP32_MATRIX = 157.3e12
PEAK_HBM = 8.0e12


def torch_route(features, weights, biases, embedding, mask, means, camera_center, n_freq):
    """The reference's formulation (gsplat_appearance_embedding_renderer.py:85-93, 261-285): gather, repeat, concat, Sequential, scatter."""
    rows = features[mask]
    parts = [rows, embedding[None].repeat(rows.shape[0], 1)]
    if n_freq:
        d = torch.nn.functional.normalize(means[mask] - camera_center, dim=-1)
        encoded = [d]
        for k in range(n_freq):
            encoded += [torch.sin(d * 2.0 ** k), torch.cos(d * 2.0 ** k)]
        parts.append(torch.cat(encoded, -1))
    x = torch.concat(parts, dim=-1)
    for i, (w, b) in enumerate(zip(weights, biases)):
        x = torch.nn.functional.linear(x, w, b)
        x = torch.relu(x) if i < len(weights) - 1 else torch.sigmoid(x)
    out = torch.zeros((features.shape[0], x.shape[1]), dtype=x.dtype, device=x.device)
    out[mask] = x
    return out


def flop_per_row(F, P, H, n_layers, n_out):
    """Multiply-adds x 2 of one pass over the layers with the embedding folded; the fused backward makes four such passes."""
    return 2 * ((F + P) * H + (n_layers - 2) * H * H + H * n_out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--workload", default="S-800-100k")
    p.add_argument("--time-limit", type=int, default=540)
    p.add_argument("--out", default=os.path.join(T.ROOT, "profiles", "appearance_mlp_time.json"))
    a = p.parse_args()
    signal.alarm(a.time_limit)
    import gspl_amd  # noqa: F401
    from gspl_amd import appearance, ops, synthetic
    from gspl_amd.renderers import HipGSplatAppearanceEmbeddingRenderer
    assert torch.cuda.is_available(), "appearance_mlp_time measures on the GPU"
    dev = torch.device("cuda:0")
    result = {"tool": "appearance_mlp_time", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
              "peak_fp32_matrix_TFs": PEAK_FP32_MATRIX / 1e12, "peak_hbm_TBs": PEAK_HBM / 1e12}
    gen = torch.Generator().manual_seed(42)
    F, E, H, L, n_out = 64, 32, 64, 3, 3
    shapes = (("N_1M_30pct_visible", 1_000_000, 0.3, 0), ("N_1M_all_visible", 1_000_000, 1.0, 0), ("N_100k_all_visible", 100_000, 1.0, 0),
              ("view_dependent_N_1M_30pct_visible", 1_000_000, 0.3, 4))
    for name, N, share, n_freq in shapes:
        P = 3 * (2 * n_freq + 1) if n_freq else 0
        model = appearance.HipAppearanceModel(appearance.ModelConfig(n_appearances=4, is_view_dependent=n_freq > 0)).to(dev)
        linears = model._linears()
        weights, biases = [m.weight for m in linears], [m.bias for m in linears]
        embedding = model.embedding.weight[1].detach().clone().requires_grad_(True)
        features = (torch.randn(N, F, generator=gen) * 0.5).to(dev).requires_grad_(True)
        mask = (torch.rand(N, generator=gen) < share).to(dev)
        means, camera_center = (torch.randn(N, 3, generator=gen) * 2).to(dev), torch.tensor([0.3, -0.2, 4.0], device=dev)
        v_out = torch.randn(N, n_out, generator=gen).to(dev)
        leaves = [features, embedding] + weights + biases
        visible = int(mask.sum())

        def clear():
            for leaf in leaves:
                leaf.grad = None

        def fused(_=0):
            clear()
            out = ops.appearance_mlp(features, weights, biases, embedding, mask=mask, means=means if n_freq else None,
                                     camera_center=camera_center if n_freq else None, n_view_frequencies=n_freq)
            out.backward(v_out)
            return out

        def restated(_=0):
            clear()
            out = torch_route(features, weights, biases, embedding, mask, means, camera_center, n_freq)
            out.backward(v_out)
            return out

        routes = {"torch": restated, "hip": fused}
        got = fused().detach()
        got_grads = [leaf.grad.clone() for leaf in leaves]
        want = restated().detach()
        worst_out = float((got - want).abs().max())
        worst_grad = max(float((g - leaf.grad).abs().max() / leaf.grad.abs().max().clamp_min(1e-30)) for g, leaf in zip(got_grads, leaves))
        del got, want, got_grads
        peak = {}
        for k, fn in routes.items():
            clear()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - base
        times = T.alternate(list(routes), lambda k, i: routes[k](i), a.repeats, a.steps, a.warmup)
        best = {k: min(v) for k, v in times.items()}
        spread = {k: max(v) - min(v) for k, v in times.items()}
        fwd_ms = T.timed(lambda i: ops.appearance_mlp(features.detach(), [w.detach() for w in weights], [b.detach() for b in biases], embedding.detach(),
                                                      mask=mask, means=means if n_freq else None, camera_center=camera_center if n_freq else None,
                                                      n_view_frequencies=n_freq), a.steps, a.warmup)
        flop = 4 * flop_per_row(F, P, H, L, n_out) * visible
        bytes_moved = visible * (2 * F + 2 * n_out) * 4 + N * (1 + n_out * 4) + (N - visible) * F * 4
        seconds = best["hip"] * 1e-3
        result[name] = {
            "rows": N, "visible_rows": visible, "view_frequencies": n_freq,
            "fwd_bwd_ms_min_of_repeats": {k: round(v, 4) for k, v in best.items()},
            "fwd_bwd_ms_spread_of_repeats": {k: round(v, 4) for k, v in spread.items()},
            "fwd_bwd_ms_repeats": {k: [round(t, 4) for t in v] for k, v in times.items()},
            "speedup": round(best["torch"] / best["hip"], 2),
            "hip_faster_beyond_spread": best["torch"] - best["hip"] > max(spread.values()),
            "fwd_only_ms_hip": round(fwd_ms, 4),
            "peak_bytes_over_inputs": peak, "hip_peak_memory_lower": peak["hip"] < peak["torch"],
            "flop_fwd_bwd_hip": flop, "achieved_TFs": round(flop / seconds / 1e12, 3), "fraction_of_fp32_matrix_peak": round(flop / seconds / PEAK_FP32_MATRIX, 4),
            "bytes_fwd_bwd_hip": bytes_moved, "achieved_TBs": round(bytes_moved / seconds / 1e12, 4), "fraction_of_hbm_peak": round(bytes_moved / seconds / PEAK_HBM, 4),
            "arithmetic_bound_ms": round(flop / PEAK_FP32_MATRIX * 1e3, 4), "bandwidth_bound_ms": round(bytes_moved / PEAK_HBM * 1e3, 4),
            "worst_out_difference": worst_out, "worst_gradient_difference_over_max": worst_grad,
        }
        del features, mask, means, v_out, leaves, model

    # (b) the plugin's step, fused against the torch path, one model
    wl = synthetic.WORKLOADS[a.workload]
    W, Himg = wl["width"], wl["height"]
    means, scales, quats, opac, shs = T.scene(wl, dev)
    model = synthetic.ModelObject(means, scales, quats, opac, shs)
    model.appearance_features = torch.nn.Parameter(torch.randn(means.shape[0], 64, device=dev) * 0.5)
    model.get_appearance_features = lambda: model.appearance_features
    camera = synthetic.CameraObject(synthetic.camera(W, Himg, wl["fx"]), dev)
    camera.appearance_id = torch.tensor(2, dtype=torch.int, device=dev)
    bg = torch.zeros(3, device=dev)
    target = torch.rand(3, Himg, W, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    plugins = {}
    for k, fused_mlp in (("torch_path", False), ("fused", True)):
        torch.manual_seed(3)
        plugin = HipGSplatAppearanceEmbeddingRenderer(model=appearance.ModelConfig(n_appearances=4), fused_mlp=fused_mlp).instantiate()
        plugin._setup_model(device=dev)
        plugin.train()
        plugins[k] = plugin

    def step(k, i):
        for leaf in list(model.parameters()) + list(plugins[k].parameters()):
            leaf.grad = None
        out = plugins[k].training_forward(10 ** 6, None, camera, model, bg)
        (out["render"] - target).abs().mean().backward()

    times = T.alternate(list(plugins), step, a.repeats, max(a.steps, 10), a.warmup + 2)
    result["plugin_step"] = {"workload": a.workload, "n": wl["n"], "width": W, "height": Himg,
                             "ms_per_step_min_of_repeats": {k: round(min(v), 4) for k, v in times.items()},
                             "ms_per_step_repeats": {k: [round(t, 4) for t in v] for k, v in times.items()},
                             "fused_over_torch_path": round(min(times["fused"]) / min(times["torch_path"]), 3),
                             "note": "forward, L1, backward; no optimizer step; the torch path evaluates every row and masks the result"}
    signal.alarm(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

"""SegAnyGS local feature smoothing and the neighbour search in front of it: `ops.smooth_features` (one launch per direction, the
[N, S, D] gather never materialised) against the reference's formulation (internal/segany_splatting.py:280-308) restated with
float32 torch ops — normalize, index, mean, normalize, autograd — on the same GPU, in one process, the two routes alternating repeat
by repeat.

Workload: `--n` points uniform in the Blender init box [-1.3, 1.3]^3, K = 16 neighbours, D = 32 features, 8 selected columns (a new
draw of `torch.randperm(16)[:8]` per step for both routes, as in training).
  (a) forward + backward of the smoothing, both routes; per repeat the MEDIAN of `--steps` runs, each between its own pair of device
      events.  Peak device memory of each route from `torch.cuda.max_memory_allocated`, over what was allocated before the route ran.
  (b) `ops.knn_points`, the cloud against itself at K = 16 (the map the reference computes once), and `ops.knn_graph` on its result.
  (c) `ops.knn_points`, 20 480 sampled rows against the cloud (the appearance-similarity regulariser's query, every 50 steps).

Traffic model of (a): the bytes that MUST move are, per Gaussian, the forward's S gathered rows and 1 written row and the backward's
mirror of it: 2 (S + 1) D 4 N bytes.  `fraction_of_8TBs` is that figure over the median time over 8e12 B/s.
  python tools/knn_smooth_time.py [--n 1000000] [--steps 5] [--warmup 2] [--repeats 3] [--out profiles/knn_smooth_time.json]"""
import argparse
import json
import os
import statistics

import _step_time as T  # noqa: F401  (puts the repository root on sys.path)
import torch


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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=os.path.join(T.ROOT, "profiles", "knn_smooth_time.json"))
    a = p.parse_args()
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    assert torch.cuda.is_available(), "knn_smooth_time measures on the GPU"
    dev = torch.device("cuda:0")
    N, K, D, S, Q = a.n, 16, 32, 8, 20480
    gen = torch.Generator().manual_seed(42)
    xyz = ((torch.rand(N, 3, generator=gen) * 2 - 1) * 1.3).to(dev)
    feats = torch.randn(N, D, generator=gen).to(dev)
    v_out = torch.randn(N, D, generator=gen).to(dev)
    rows = torch.randperm(N, generator=gen)[:min(Q, N)].to(dev)
    queries = xyz[rows].contiguous()

    # (b), (c): the searches
    knn_self_ms = _median_ms(lambda: ops.knn_points(xyz[None], xyz[None], K=K), a.steps, a.warmup)
    knn_sampled_ms = _median_ms(lambda: ops.knn_points(queries[None], xyz[None], K=K), a.steps, a.warmup)
    idx = ops.knn_points(xyz[None], xyz[None], K=K).idx[0]
    sampled = ops.knn_points(queries[None], xyz[None], K=K)
    assert torch.equal(sampled.idx[0], idx[rows]) and torch.equal(idx[:, 0], torch.arange(N, device=dev))
    graph_ms = _median_ms(lambda: ops.knn_graph(idx), a.steps, a.warmup)
    graph = ops.knn_graph(idx)
    longest = int((graph.row_start[1:] - graph.row_start[:-1]).max())
    del sampled

    draws = torch.Generator().manual_seed(7)

    def kernel():
        x = feats.detach().requires_grad_(True)
        ops.smooth_features(x, graph, torch.randperm(K, generator=draws)[:S]).backward(v_out)
        return x.grad

    def restated():
        x = feats.detach().requires_grad_(True)
        n = torch.nn.functional.normalize(x, dim=-1, p=2)
        m = n[idx[:, torch.randperm(K, generator=draws)[:S]], :].mean(dim=1)
        (m / (m.norm(dim=-1, keepdim=True) + 1e-9)).backward(v_out)
        return x.grad

    # the two routes compute the same thing at the size that is timed
    draws.manual_seed(7)
    gk = kernel()
    draws.manual_seed(7)
    gr = restated()
    rms = float(gr.square().mean().sqrt())
    worst_grad = float(((gk - gr).abs() / (gr.abs() + rms)).max())
    del gk, gr
    routes = {"restated": restated, "kernel": kernel}
    medians = {name: [] for name in routes}
    peaks = {name: 0 for name in routes}
    for rep in range(a.repeats):
        for name in (list(routes) if rep % 2 == 0 else list(routes)[::-1]):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            medians[name].append(_median_ms(routes[name], a.steps, a.warmup))
            peaks[name] = max(peaks[name], torch.cuda.max_memory_allocated() - before)
    med = {k: statistics.median(v) for k, v in medians.items()}
    bytes_moved = 2 * (S + 1) * D * 4 * N
    result = {
        "tool": "knn_smooth_time", "points": N, "K": K, "D": D, "selected_columns": S, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
        "device": torch.cuda.get_device_name(0),
        "smooth_fwd_bwd_ms_median_of_repeats": {k: round(v, 4) for k, v in med.items()},
        "smooth_fwd_bwd_ms_repeats": {k: [round(x, 4) for x in v] for k, v in medians.items()},
        "speedup": round(med["restated"] / med["kernel"], 2),
        "kernel_faster_beyond_spread": max(medians["kernel"]) < min(medians["restated"]),
        "peak_bytes_over_inputs": peaks, "peak_bytes_saved": peaks["restated"] - peaks["kernel"],
        "peak_ratio_restated_over_kernel": round(peaks["restated"] / max(peaks["kernel"], 1), 2),
        "gather_bytes_the_restatement_materialises": N * S * D * 4,
        "smooth_bytes_that_must_move": bytes_moved, "smooth_GBs": round(bytes_moved / (med["kernel"] * 1e-3) / 1e9, 1),
        "fraction_of_8TBs": round(bytes_moved / (med["kernel"] * 1e-3) / 8e12, 4),
        "worst_gradient_difference_over_abs_plus_rms": worst_grad,
        "knn_points_self_query_ms": round(knn_self_ms, 4), "knn_points_sampled_queries": int(queries.shape[0]),
        "knn_points_sampled_ms": round(knn_sampled_ms, 4), "knn_graph_ms": round(graph_ms, 4), "longest_inverse_list": longest,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

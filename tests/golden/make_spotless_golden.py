"""
make_spotless_golden.py — generates tests/golden/ref_spotless.npz by IMPORTING the reference's own torch code
(internal/metrics/spotless_metrics.py: `SpotLessModule`, `SpotLessMetricsModule`) where its tree is present, through the `lightning`
stand-in of tests/lightning_standin.py.

Run from the repo root:   python tests/golden/make_spotless_golden.py <path to the reference tree>
Its output is committed; nothing under tests/ reads the reference tree at test time (but tests/spotless_reference_worker.py).

Fixture (ref_spotless.npz)
  state/*                    a seeded `SpotLessModule` with C = 24 features (+ 80 of the positional encoding), as float64
  sf [24, 5, 7]              the feature map; the image is 13 x 11
  render, gt [3, 13, 11]     a seeded frame; lower_thr, upper_thr the two thresholds the masks below were taken at
  pe32 [13, 11, 80]          the float32 `get_positional_encodings(13, 11, 20)`; pe32_9 [9, 9, 80] the one of the resizing branch
  mask64 / mask32, up64 / up32        `mlp_mask`'s pred_mask and pred_mask_up without resizing, in float64 and in float32
  mask64_r / mask32_r, up64_r / up32_r   the same with max_mlp_mask_size = 9 (a 9 x 9 mask resampled to 13 x 11)
  lower_mask, upper_mask     `robust_mask` of the frame's error at the two thresholds, [1, 13, 11, 1]
  spot64, reg64, grad64/*    the spot loss, 0.5 x the regulariser and the float64 gradients of the four parameters; *_r: resizing branch
  err_map [1, 13, 11, 3], robust_a, robust_b, thr_a, thr_b   `robust_mask` on a seeded error map at two thresholds
  stats_render, stats_gt [3, 3, 13, 11]; stats_counts [3, 50]; stats_hist [3, 50]; stats_avg, stats_lower, stats_upper [3]
                             three consecutive `update_running_stats` steps at bin_size = 50 and what they left
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
C, H0, W0, H, W = 24, 5, 7, 13, 11


def build(spotless, max_mlp_mask_size, bin_size=50):
    cfg = spotless.SpotLessMetrics(n_feature_dims=C, bin_size=bin_size, max_mlp_mask_size=max_mlp_mask_size)
    module = cfg.instantiate()
    module.setup("fit", None)
    module.training_setup(types.SimpleNamespace(on_after_backward_hooks=[]))
    return module


def main(reference):
    sys.path.insert(0, TESTS)
    sys.path.insert(0, reference)
    import lightning_standin
    lightning_standin.install()
    import internal.metrics.spotless_metrics as spotless

    g = torch.Generator().manual_seed(20241)
    torch.manual_seed(20241)
    module = build(spotless, 800)
    state = {k: v.clone() for k, v in module.spotless_module.state_dict().items()}
    sf = torch.randn(C, H0, W0, generator=g)
    gt = torch.rand(3, H, W, generator=g)
    render = (gt + 0.35 * torch.randn(3, H, W, generator=g) * (torch.rand(1, H, W, generator=g) > 0.5)).clamp(0, 1)
    lower_thr, upper_thr = 0.05, 0.2
    data = {"sf": sf, "render": render, "gt": gt, "lower_thr": torch.tensor(lower_thr), "upper_thr": torch.tensor(upper_thr),
            "pe32": module.get_positional_encodings(H, W, 20, device="cpu"), "pe32_9": module.get_positional_encodings(9, 9, 20, device="cpu")}
    data.update({"state/" + k: v.double() for k, v in state.items()})

    for tag, size in (("", 800), ("_r", 9)):
        for bits, dtype in (("32", torch.float32), ("64", torch.float64)):
            m = build(spotless, size).to(dtype)
            m.spotless_module.load_state_dict({k: v.to(dtype) for k, v in state.items()})
            m._lower_err.fill_(lower_thr)
            m._upper_err.fill_(upper_thr)
            error = torch.abs(render - gt).permute(1, 2, 0).unsqueeze(0)      # float32 in both runs: `robust_mask` takes no other
            up, mask, lower_mask, upper_mask = m.mlp_mask(sf.to(dtype).unsqueeze(0), error, height=H, width=W)
            data["mask" + bits + tag], data["up" + bits + tag] = mask.detach(), up.detach()
            if bits == "64":
                spot = m.spotless_loss(up.flatten(), upper_mask.flatten(), lower_mask.flatten())
                data["spot64" + tag], data["reg64" + tag] = spot.detach(), 0.5 * m.spotless_module.get_regularizer()
                spot.backward()
                data.update({"grad64" + tag + "/" + k: p.grad for k, p in m.spotless_module.named_parameters()})
                if tag == "":
                    data["lower_mask"], data["upper_mask"] = lower_mask.float(), upper_mask.float()

    err_map = torch.rand(1, H, W, 3, generator=g) * torch.rand(1, H, W, 1, generator=g)
    thr_a, thr_b = 0.12, 0.3
    data.update({"err_map": err_map, "thr_a": torch.tensor(thr_a), "thr_b": torch.tensor(thr_b),
                 "robust_a": spotless.SpotLessMetricsModule.robust_mask(err_map, thr_a),
                 "robust_b": spotless.SpotLessMetricsModule.robust_mask(err_map, thr_b)})

    m = build(spotless, 800)
    rows = {k: [] for k in ("render", "gt", "counts", "hist", "avg", "lower", "upper")}
    for step in range(3):
        gt_s = torch.rand(3, H, W, generator=g)
        render_s = (gt_s + (0.1 + 0.2 * step) * torch.randn(3, H, W, generator=g)).clamp(0, 1)
        m.update_running_stats({"render": render_s}, (None, ("frame", gt_s, None), None), None, step, None)
        predict, gt_image = render_s.permute(1, 2, 0).unsqueeze(0), gt_s.permute(1, 2, 0).unsqueeze(0)      # as the reference forms them
        counts = torch.histogram(torch.mean(torch.abs(predict - gt_image), dim=-1).clone(), bins=50, range=(0.0, 1.0))[0]
        for k, v in zip(rows, (render_s, gt_s, counts, m._hist_err.clone(), m._avg_err.clone(), m._lower_err.clone(), m._upper_err.clone())):
            rows[k].append(v)
    data.update({"stats_" + k: torch.stack(v) for k, v in rows.items()})

    out = os.path.join(HERE, "ref_spotless.npz")
    np.savez_compressed(out, **{k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in data.items()})
    print("wrote ref_spotless.npz", os.path.getsize(out), "bytes,", len(data), "arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "internal", "metrics", "spotless_metrics.py")):
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))

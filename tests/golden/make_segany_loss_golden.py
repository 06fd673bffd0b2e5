"""
make_segany_loss_golden.py — generates tests/golden/ref_segany_loss.npz by IMPORTING the reference's own torch code
(internal/segany_splatting.py: `SegAnySplatting.mask_preprocess` and `forward_with_loss_calculation`) where its tree is present,
through the `lightning` stand-in of tests/lightning_standin.py and `gspl_amd.compat.install()`.

Run from the repo root:   python tests/golden/make_segany_loss_golden.py <path to the reference tree>
Its output is committed; nothing under tests/ reads the reference tree at test time.

The two unbound methods are called on a stand-in `self`, on the CPU; `Tensor.cuda` is the identity inside this process only, `q_trans`
is the fixed monotone function s / (1 + s), the renderer's output is a seeded float64 map and `rfn` is 0, so the loss is the
correspondence loss alone.  `mask_preprocess` runs in float32 where the reference casts to it (`sam_masks.float()`); everything behind
it runs in float64.  Every random draw is recorded.

Fixture (ref_segany_loss.npz)
  masks [12, 13, 11] u8, mask_scales [12] f32, upper_bound_scale, ray_sample_rate
  rendered [8, 7, 5] f64 (the renderer's map: C = 8), gate_weight [8, 1], gate_bias [8] f64 (the `scale_gate` Linear)
  draw_randperm [12], draw_rand_hw [13, 11], draw_rand1 [11] (the scale in front, then one per sampled scale), draw_rand_ss [S, S] f32
  sampled_ray [13, 11] bool, per_pixel_weight [S, S] f32, gt_corrs [10, S, S] u8, sampled_scales [10] f64 (behind q_trans)
  gates [10, 8] f64, loss, cosine_pos, cosine_neg f64
  grad_rendered [8, 7, 5], grad_gates [10, 8], grad_gate_weight [8, 1], grad_gate_bias [8] f64
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
N, H, W, C, HR, WR = 12, 13, 11, 8, 7, 5


def frame(g):
    """Overlapping rectangles of several sizes (some pixels stay uncovered, some pairs share no mask); scales grow with the area."""
    masks = torch.zeros(N, H, W, dtype=torch.uint8)
    for i in range(N):
        h, w = int(torch.randint(2, 9, (1,), generator=g)), int(torch.randint(2, 8, (1,), generator=g))
        y, x = int(torch.randint(0, H - h + 1, (1,), generator=g)), int(torch.randint(0, W - w + 1, (1,), generator=g))
        masks[i, y:y + h, x:x + w] = 1
    scales = masks.flatten(1).sum(1).float().sqrt() * (0.9 + 0.2 * torch.rand(N, generator=g))
    shuffle = torch.randperm(N, generator=g)
    return masks[shuffle].contiguous(), scales[shuffle].contiguous()


def main(reference):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, TESTS)
    sys.path.insert(0, reference)
    import lightning_standin
    lightning_standin.install()
    from gspl_amd import compat
    compat.install()
    from internal.segany_splatting import SegAnySplatting

    torch.Tensor.cuda = lambda self, *args, **kwargs: self
    g = torch.Generator().manual_seed(20251)
    torch.manual_seed(20251)
    masks, scales = frame(g)
    rendered = torch.randn(C, HR, WR, generator=g, dtype=torch.float64).requires_grad_(True)
    gate = torch.nn.Sequential(torch.nn.Linear(1, C, bias=True), torch.nn.Sigmoid()).double()
    kept = {}
    gate.register_forward_hook(lambda module, args, out: (out.retain_grad(), kept.__setitem__("gates", out))[0])

    class StandIn:
        upper_bound_scale = float(scales.max())
        ray_sample_rate = 0.3
        num_sampled_rays = 1000
        scale_aware_dim = -1
        rfn = 0.0
        scale_gate = gate

        @staticmethod
        def q_trans(s):
            return (s / (1 + s)).reshape(-1, 1).double()

        def __call__(self, camera):
            return {"render": rendered}

    self = StandIn()
    draws = {"rand": [], "randperm": [], "rand_like": []}
    real = {name: getattr(torch, name) for name in draws}

    def recorded(name):
        def call(*args, **kwargs):
            out = real[name](*args, **kwargs)
            draws[name].append(out.clone())
            return out
        return call

    for name in draws:
        setattr(torch, name, recorded(name))
    preprocessed = {}

    def mask_preprocess(sam_masks, mask_scales):
        out = SegAnySplatting.mask_preprocess(self, sam_masks=sam_masks, mask_scales=mask_scales)
        preprocessed["out"] = out
        return out

    self.mask_preprocess = mask_preprocess
    try:
        _, loss, cosine_pos, cosine_neg, _ = SegAnySplatting.forward_with_loss_calculation(self, None, None, (masks, scales))
    finally:
        for name in draws:
            setattr(torch, name, real[name])
    loss.backward()
    sampled_ray, per_pixel_weight, gt_corrs, sampled_scales = preprocessed["out"]
    assert len(draws["randperm"]) == 1 and len(draws["rand_like"]) == 1 and tuple(draws["rand"][0].shape) == (H, W) and len(draws["rand"]) == 12
    assert per_pixel_weight.dtype == torch.float32 and gt_corrs.dtype == torch.float32
    weight, bias = gate[0].weight, gate[0].bias
    data = {"masks": masks, "mask_scales": scales, "upper_bound_scale": torch.tensor(self.upper_bound_scale, dtype=torch.float64),
            "ray_sample_rate": torch.tensor(self.ray_sample_rate, dtype=torch.float64), "rendered": rendered, "gate_weight": weight, "gate_bias": bias,
            "draw_randperm": draws["randperm"][0], "draw_rand_hw": draws["rand"][0], "draw_rand1": torch.cat(draws["rand"][1:]),
            "draw_rand_ss": draws["rand_like"][0], "sampled_ray": sampled_ray, "per_pixel_weight": per_pixel_weight, "gt_corrs": gt_corrs.to(torch.uint8),
            "sampled_scales": sampled_scales, "gates": kept["gates"], "loss": loss, "cosine_pos": cosine_pos, "cosine_neg": cosine_neg,
            "grad_rendered": rendered.grad, "grad_gates": kept["gates"].grad, "grad_gate_weight": weight.grad, "grad_gate_bias": bias.grad}
    out = os.path.join(HERE, "ref_segany_loss.npz")
    np.savez_compressed(out, **{k: v.detach().numpy() for k, v in data.items()})
    total = gt_corrs.sum(0)
    print("wrote ref_segany_loss.npz", os.path.getsize(out), "bytes,", len(data), "arrays; S =", int(sampled_ray.sum()), "loss", float(loss.detach()),
          "pairs labelled at no / every scale:", int((total == 0).sum()), int((total == 10).sum()))


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "internal", "segany_splatting.py")):
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))

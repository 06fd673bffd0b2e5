"""The density controllers' opacity reset as the GPU tests restate it (`hip_helpers.reset_opacities`): the vanilla, 2DGS and Taming
controllers set every opacity to min(o, 0.01) every 3000 steps, through the model's inverse sigmoid and sigmoid in fp32."""
import numpy as np
import torch

from hip_helpers import RESET_OPACITY, reset_opacities


def test_reset_opacities_matches_the_reference_in_fp32():
    o = torch.tensor([0.9, 0.5, 0.0100001, 0.01, 0.0099999, 0.005, 1.0 / 255.0, 1e-4], dtype=torch.float32)
    r = reset_opacities(o)
    assert r.dtype == torch.float32
    # inverse_sigmoid(0.01) then sigmoid, in fp32: one ulp below 0.01 (0.0099999988)
    assert float(r[0]) == RESET_OPACITY and np.float32(RESET_OPACITY) == np.float32(0.0099999988)
    assert torch.all(r[:4] == r[0])
    # below the reset value no clamp: the opacity goes through the same fp32 round trip, a few ulps at most
    low = o[4:]
    x = low.clone()
    assert torch.equal(r[4:], torch.sigmoid(torch.log(x / (1 - x))))
    assert torch.all((r[4:] - low).abs() <= 4 * torch.finfo(torch.float32).eps * low)
    assert torch.all(r[4:] < r[0])
    # and a different reset value
    assert torch.equal(reset_opacities(torch.tensor([0.5]), value=0.05), torch.sigmoid(torch.log(torch.tensor([0.05]) / (1 - torch.tensor([0.05])))))

"""The depth-regularisation loss on the GPU (csrc/depthloss.hip, `ops.depth_loss`) against the fp64 torch restatement that the CPU path
of the same op is (pinned to the reference's modules by tests/test_depthreg.py): every kind x normalisation x mask combination at
67 x 45 (two partial sums, the last one ragged) and at 1 x 1, with counted float32 bounds, and two runs bit-equal."""
import pytest
import torch

import gspl_amd  # noqa: F401
from gspl_amd import _lib as L
from gspl_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# ---- the depth loss ----------------------------------------------------------------------------------------------------------------------
EPS = 2.0 ** -24


def _depth_inputs(H, W):
    g = torch.Generator().manual_seed(7 + H)
    pred, gt = torch.rand(H, W, generator=g) * 3 + 0.05, torch.rand(H, W, generator=g) * 3 + 0.05
    gt_mask = (torch.rand(H, W, generator=g) > 0.2).float() * (0.5 + torch.rand(H, W, generator=g))      # a weight map, zeros included
    pixel_mask = torch.rand(H, W, generator=g) > 0.3
    return pred, gt, gt_mask, pixel_mask


def _fp64_parts(pred, gt, normalize, median, m1, m2):
    """gt', pred' and d pred' / d pred of the reference's operations, in float64."""
    pn, gn = pred.double(), gt.double()
    scale = torch.ones_like(pn)
    if normalize == "minmax":
        den = pn.max() - pn.min() + 1e-8
        pn, scale = (pn - pn.min()) / den, scale / den
    elif normalize == "median":
        pn, scale = pn / median.double(), scale / median.double()
    elif normalize == "mean":
        mean = gn.mean()
        pn, gn, scale = pn / mean, gn / mean, scale / mean
    for m in (m1, m2):
        if m is not None:
            pn, gn, scale = pn * m.double(), gn * m.double(), scale * m.double()
    return gn, pn, scale


@pytest.mark.parametrize("masks", ["none", "gt", "pixel", "both"])
@pytest.mark.parametrize("normalize", [None, "minmax", "median", "mean"])
@pytest.mark.parametrize("kind", ["l1", "l2"])
@pytest.mark.parametrize("hw", [(45, 67), (1, 1)], ids=["67x45", "1x1"])
def test_depth_loss_against_fp64(hw, kind, normalize, masks):
    """Counted float32 bounds, u = 2^-24, s = |gt'| + |pred'| per element, d = gt' - pred'.
      sums     a chain of 8 per thread, a butterfly of 6 levels, 3 adds over the waves; the second level the same over the partials (2 here);
               a division: at most S = 32 roundings, S u sum|terms|.
      inputs   pred': the subtraction, the denominator (its subtraction, its addition, float32's 1e-8), the division, two masks: at
               most 8 roundings; gt' fewer; the difference one more: |d_fp32 - d| <= R u s with R = 9, and R = 9 + S with the mean
               normalisation, whose divisor is itself a float32 sum of positive terms.
      loss     L1: each term moves by R u s; L2: by 2 |d| R u s + u d^2 (second-order terms are below 1e-12 of these).
      gradient -(sign d or 2 d) (d pred' / d pred) grad / (H W): the same R roundings relative to the reference where L1's sign is firm
               (|d| > R u s); L2 adds 2 R u s (d pred' / d pred) grad / (H W).  Where the sign is not firm, L1's gradient is bounded by its size.
    minmax at 1 x 1 divides 0 by 1e-8: exactly 0 on both sides."""
    H, W = hw
    pred, gt, gt_mask, pixel_mask = _depth_inputs(H, W)
    median = torch.median(gt[gt > 0]) if normalize == "median" else None
    m1 = gt_mask if masks in ("gt", "both") else None
    m2 = pixel_mask if masks in ("pixel", "both") else None
    p64 = pred.double().requires_grad_(True)
    ref = ops.depth_loss(p64, gt.double(), kind, normalize, None if median is None else median.double(), None if m1 is None else m1.double(), m2)
    ref.backward()
    S, R = 32, 9 + (32 if normalize == "mean" else 0)
    gn, pn, scale = _fp64_parts(pred, gt, normalize, median, m1, m2)
    s, d = gn.abs() + pn.abs(), gn - pn
    terms = d.abs() if kind == "l1" else d * d
    assert abs(float(terms.mean()) - float(ref.detach())) <= 1e-12 * max(1.0, abs(float(ref.detach())))
    term_err = R * EPS * s if kind == "l1" else 2 * d.abs() * R * EPS * s + EPS * d * d
    bound = float((term_err.sum() + S * EPS * terms.sum()) / (H * W)) + 1e-45

    p = pred.to(DEV).requires_grad_(True)
    args = (gt.to(DEV), kind, normalize, median, None if m1 is None else m1.to(DEV), None if m2 is None else m2.to(DEV))
    got = ops.depth_loss(p, *args)
    assert got.shape == () and got.dtype == torch.float32
    err = abs(float(got.detach()) - float(ref.detach()))
    print(f"loss {float(ref.detach()):.6e}: |got - ref| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    (got * 1.5).backward()
    g_ref, unit = 1.5 * p64.grad, 1.5 * scale.abs() / (H * W)      # unit: the size of L1's gradient
    g_err = (p.grad.cpu().double() - g_ref).abs()
    if kind == "l1":
        firm = d.abs() > R * EPS * s
        assert bool((g_err[firm] <= (R * EPS * g_ref.abs() + 1e-45)[firm]).all()), float(g_err[firm].max())
        assert bool((g_err[~firm] <= (2 * unit * (1 + R * EPS))[~firm]).all())
    else:
        assert bool((g_err <= R * EPS * g_ref.abs() + 2 * R * EPS * s * unit + 1e-45).all()), float(g_err.max())

    # two runs: the same bits, loss and gradient
    p2 = pred.to(DEV).requires_grad_(True)
    again = ops.depth_loss(p2, *args)
    (again * 1.5).backward()
    assert torch.equal(again, got) and torch.equal(p2.grad, p.grad)


def test_depth_loss_median_on_the_device_mask_dtypes_and_refusals():
    """A median on the device is read there; a pixel mask as bytes, bools or floats of 0 / 1 gives the same bits; `l1+ssim` is refused
    with the reason, an unknown kind by the library."""
    pred, gt, gt_mask, pixel_mask = (t.to(DEV) for t in _depth_inputs(45, 67))
    median = torch.median(gt[gt > 0])
    assert median.is_cuda
    on_device = ops.depth_loss(pred, gt, "l1", "median", median)
    by_value = ops.depth_loss(pred, gt, "l1", "median", float(median))
    assert torch.equal(on_device, by_value)
    u8, as_bool = ops.depth_loss(pred, gt, "l2", None, None, gt_mask, pixel_mask.to(torch.uint8)), ops.depth_loss(pred, gt, "l2", None, None, gt_mask, pixel_mask)
    as_float = ops.depth_loss(pred, gt, "l2", None, None, gt_mask, pixel_mask.float())
    assert torch.equal(u8, as_bool) and torch.equal(u8, as_float)
    with pytest.raises(NotImplementedError, match="torchmetrics"):
        ops.depth_loss(pred, gt, "l1+ssim")
    rc = L.lib().gspl_depth_loss_fwd(45, 67, 7, 0, L.ptr(pred), L.ptr(gt), None, 0.0, None, 0, None, 0, L.ptr(pred), 1 << 20, L.ptr(pred), None)
    assert rc == L.GSPL_ERR_UNSUPPORTED

"""The SpotLess ops (include/gspl_hip.h section 23, csrc/spotless.hip, ops/spotless.py) against the fp64 oracle tests/spotless_oracle.py,
which tests/test_spotless_cpu.py pins to the reference's own run.

Tolerances.  eps32 = 2^-23 (one ulp of 1.0; a rounded operation errs by at most half of it, so every count below has a factor 2 of room
for second-order terms).  The oracle forms the resampling indices and weights in float32 exactly as the kernels do, so they carry no
error of their own, and it returns with every sum the sum of the absolute terms it is made of.

  forward   A term of z passes 6 rounded operations: its product with the column weight, the column combine, the product with the row
            weight, the row combine, + A, + B (Z_ROUNDINGS).  The chain b2 + sum_c w2[c] relu(z[c]) is 16 fmaf: at most 16 more
            (Y_ROUNDINGS = 22).  With y_abs = |b2| + sum_c |w2[c]| z_abs[c] the value in front of the sigmoid errs by at most
            22 eps32 y_abs; the sigmoid's slope is at most 1/4; expf (2 ulp), 1 + e and the division add 4 eps32 of a value <= 1:
                |out - ref| <= 22 eps32 y_abs / 4 + 4 eps32
            and with the second resampling the same bound resampled (the weights are non-negative and sum to 1) + 4 eps32 for its two
            products and two combines.
  backward  |v - ref| <= eps32 (TERM_ROUNDINGS + chain) v_abs + v_fragile, v_abs the oracle's sum of the absolute terms.
            A term dy w2[c] (times the two adjoint weights for v_G) carries: the slope e / (1 + e)^2 from e = expf(-|y|) (2 ulp), 1 + e,
            the square and the division: 5 operations; v times the slope; times w2; the two adjoint weights: 9, counted as
            TERM_ROUNDINGS = 10.  v_w2's term dy relu(z) carries the 6 roundings of z besides, and its absolute terms are those of z.
            The longest addition chain, per output (`_chains`; counted from the resampling's own index tables):
              v_G   the mask rows that read one row of G (a lane's chain) + the mask columns that read one column of G (the final kernel)
              v_A   the 6 steps of the butterfly over a wave's 64 columns + the column blocks
              v_B   the mask rows one row of G owns (a lane's chain) + the rows of G
              v_w2, v_b2   the owned rows + a butterfly (6) + the (row of G, column block) partials per lane of the final wave + a butterfly (6)
            and with the second resampling the gather of v adds the output rows + the output columns that read one mask pixel.
            In the large case, (50, 50) -> (70, 90) -> (100, 61), these come to 13, 14, 58 and 22 additions.
  fragile   A hidden unit with |z| <= 6 eps32 z_abs may fall on the other side of the relu in float32: its whole term is added to the
            tolerance of the sums it feeds (`_fragile`).  test_fragile_units_are_rare asserts that such units are fewer than 1e-4 of all
            (pixel, unit) pairs in the recipe the other tests draw their large case from, so the allowance cannot hide a wrong kernel.
The GPU tests never widen these."""
import functools

import numpy as np
import pytest
import torch

import spotless_oracle as SO
from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)

DEV = "cuda:0"
EPS = SO.EPS32
TERM_ROUNDINGS = 10

#        (h0, w0)   (mh, mw)   out_size
SHAPES = [((5, 7), (13, 11), None),
          ((5, 7), (13, 11), (17, 19)),         # up-sampling
          ((5, 7), (13, 11), (12, 5)),          # down-sampling along one axis (both here: 13 -> 12, 11 -> 5)
          ((2, 2), (2, 3), None),
          ((50, 50), (70, 90), (100, 61))]      # crosses workgroup tiles and column blocks; 90 -> 61 is a down-sampling


def _tables(h0, w0, mh, mw, seed):
    """Seeded tables; at (50, 50) the recipe of the fragile-unit count: randn features with C = 1280 through nn.Linear's default
    initialisation, A and B as 0.3 randn."""
    g = torch.Generator().manual_seed(seed)
    if (h0, w0) == (50, 50):
        torch.manual_seed(seed)
        first, second = torch.nn.Linear(1280 + 80, 16), torch.nn.Linear(16, 1)
        sf = torch.randn(1280, h0, w0, generator=g)
        with torch.no_grad():
            G = (sf.reshape(1280, -1).t() @ first.weight[:, :1280].t()).reshape(h0, w0, 16)
            w2, b2 = second.weight.reshape(16).clone(), second.bias.clone()
    else:
        G = torch.randn(h0, w0, 16, generator=g)
        w2, b2 = torch.randn(16, generator=g) * 0.5, torch.randn(1, generator=g) * 0.2
    A, B = 0.3 * torch.randn(mh, 16, generator=g), 0.3 * torch.randn(mw, 16, generator=g)
    return [t.contiguous().numpy() for t in (G, A, B, w2, b2)]


def _v_out(shape, seed):
    """About half of the pixels carry no gradient, as the spot loss has it where the two robust masks disagree."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) * (rng.random(shape) > 0.5)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(index):
    (h0, w0), (mh, mw), out_size = SHAPES[index]
    tables = _tables(h0, w0, mh, mw, 100 + index)
    v_out = _v_out(out_size or (mh, mw), 200 + index)
    return tables, v_out, SO.mask(*tables, out_size, v_out)


def _gpu(tables, out_size, v_out=None):
    from gspl_amd import ops
    dev = [torch.from_numpy(t).to(DEV) for t in tables]
    out = ops.spotless_mask_forward(*dev, out_size=out_size)
    if v_out is None:
        return out.cpu().numpy(), None
    grads = ops.spotless_mask_backward(*dev, torch.from_numpy(v_out).to(DEV), out_size=out_size)
    return out.cpu().numpy(), [g.cpu().numpy() for g in grads]


def _within(got, ref, bound, what):
    diff = np.abs(np.asarray(got, dtype=np.float64) - ref)
    ratio = diff / np.maximum(bound, 1e-300)
    print(f"{what}: worst |diff| {diff.max():.3e}, worst |diff| / bound = {ratio.max():.3f}")
    worst = np.unravel_index(np.argmax(diff - bound), diff.shape)
    assert (diff <= bound).all(), f"{what}: |diff| {diff[worst]:.3e} > bound {np.broadcast_to(bound, diff.shape)[worst]:.3e} at {worst}"


def _readers(I, O):
    """Of an axis resampled from I to O entries: the most outputs whose upper source is one source (it owns them), and the most outputs
    that read one source at all."""
    i0, i1, _, _ = SO.resample_axis(I, O)
    owned = np.bincount(i0, minlength=I)
    return int(owned.max()), int((owned + np.bincount(i1[i1 != i0], minlength=I)).max())


def _chains(tables, out_size):
    """The longest addition chain behind each gradient (the module's docstring)."""
    (h0, w0, _), mh, mw = tables[0].shape, tables[1].shape[0], tables[2].shape[0]
    (rows_owned, rows_any), (_, cols_any) = _readers(h0, mh), _readers(w0, mw)
    blocks = -(-mw // 64)
    gather = _readers(mh, out_size[0])[1] + _readers(mw, out_size[1])[1] if out_size else 0
    sums = rows_owned + 6 + -(-h0 * blocks // 64) + 6 + gather
    return {"v_G": rows_any + cols_any + gather, "v_A": 6 + blocks + gather, "v_B": rows_owned + h0 + gather, "v_w2": sums, "v_b2": sums}


def _check_gradients(grads, ref, chains, fragile=True):
    v_G, v_A, v_B, v_w = grads
    for name, got in (("v_G", v_G), ("v_A", v_A), ("v_B", v_B), ("v_w2", v_w[:16]), ("v_b2", v_w[16:])):
        roundings = TERM_ROUNDINGS + (SO.Z_ROUNDINGS if name == "v_w2" else 0)
        bound = EPS * (roundings + chains[name]) * ref[name + "_abs"] + (ref[name + "_fragile"] if fragile else 0.0)
        _within(got, ref[name], bound, name)
        assert np.abs(ref[name]).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(SHAPES)))
def test_mask_forward_and_backward_meet_the_counted_bounds(index):
    tables, v_out, ref = _case(index)
    out_size = SHAPES[index][2]
    out, grads = _gpu(tables, out_size, v_out)
    assert out.shape == (out_size or SHAPES[index][1])
    _within(out, ref["out"], ref["out_bound"], "out")
    _check_gradients(grads, ref, _chains(tables, out_size))


def test_fragile_units_are_rare():
    """The float64 reference of the recipe at (50, 50) -> (70, 90): fragile (pixel, unit) pairs are fewer than 1e-4 of all."""
    _, _, ref = _case(len(SHAPES) - 1)
    fragile, pairs = int(ref["fragile"].sum()), ref["fragile"].size
    print(f"fragile pairs: {fragile} of {pairs}")
    assert pairs == 70 * 90 * 16 and fragile < 1e-4 * pairs
    assert 0.2 < (ref["z"] > 0).mean() < 0.8           # both sides of the relu are exercised


@pytest.mark.gpu
def test_mask_exact_case_with_zero_pre_activations():
    """Integer tables and a 2x up-sampling (weights 1/4, 3/4): every z is exactly representable, and many are exactly 0.  The hidden
    gradient must be exactly 0 there, as relu's backward in torch has it."""
    from gspl_amd import ops
    rng = np.random.default_rng(5)
    h0, w0 = 3, 4
    mh, mw = 2 * h0, 2 * w0
    G = (rng.integers(-3, 4, size=(h0, w0, 16)) * 16).astype(np.float32)
    A = (rng.integers(-2, 3, size=(mh, 16)) * 16).astype(np.float32)
    B = (rng.integers(-2, 3, size=(mw, 16)) * 16).astype(np.float32)
    G[:, :, 0] = 0                                      # unit 0: z = A[i] + B[j], exactly 0 on all of row 2 ...
    A[:, 0] = (np.arange(mh) - 2) * 16
    B[:, 0] = 0
    G[:, :, 1] = 32                                     # unit 1: a constant map, cancelled exactly by A on the rows 0 and 3
    A[:, 1] = np.where(np.isin(np.arange(mh), (0, 3)), -32, 16)
    B[:, 1] = 0
    w2 = (rng.integers(1, 4, size=16) / 64).astype(np.float32)
    b2 = np.array([-0.25], dtype=np.float32)
    v_out = np.ones((mh, mw), dtype=np.float32)
    tables = [G, A, B, w2, b2]
    ref = SO.mask(*tables, None, v_out)
    assert (ref["z"][2, :, 0] == 0).all() and (ref["z"][[0, 3], :, 1] == 0).all() and (ref["z"] == 0).sum() >= 3 * mw
    assert (ref["z"] == np.round(ref["z"] * 16) / 16).all() and not ref["fragile"][ref["z"] != 0].any()
    dev = [torch.from_numpy(t).to(DEV) for t in tables]
    out = ops.spotless_mask_forward(*dev).cpu().numpy()
    v_G, v_A, v_B, v_w = (g.cpu().numpy() for g in ops.spotless_mask_backward(*dev, torch.from_numpy(v_out).to(DEV)))
    _within(out, ref["out"], ref["out_bound"], "out")
    assert v_A[2, 0] == 0 and (v_A[[0, 3], 1] == 0).all(), "a unit with z == 0 let a gradient through"
    assert v_A[3, 0] != 0 and v_A[1, 1] != 0
    # exactly 0 wherever the oracle's sum has no term at all, in every gradient
    for got, name in ((v_G, "v_G"), (v_A, "v_A"), (v_B, "v_B")):
        assert not got[ref[name + "_abs"] == 0].any(), name
    _check_gradients((v_G, v_A, v_B, v_w), ref, _chains(tables, None), fragile=False)      # z is exact: no unit is on the wrong side


@pytest.mark.gpu
def test_mask_backward_is_deterministic_and_zero_for_a_zero_gradient():
    from gspl_amd import ops
    index = len(SHAPES) - 1
    tables, v_out, _ = _case(index)
    out_size = SHAPES[index][2]
    dev = [torch.from_numpy(t).to(DEV) for t in tables]
    v = torch.from_numpy(v_out).to(DEV)
    first = [g.clone() for g in ops.spotless_mask_backward(*dev, v, out_size=out_size)]
    second = ops.spotless_mask_backward(*dev, v, out_size=out_size)
    assert all(torch.equal(a, b) for a, b in zip(first, second)), "two backward runs differ in their bits"
    assert all(bool(g.any()) for g in first)
    for size in (out_size, None):
        shape = size or SHAPES[index][1]
        poisoned = [torch.full_like(g, float("nan")) for g in first]
        zero = ops.spotless_mask_backward(*dev, torch.zeros(shape, device=DEV), size, *poisoned)
        assert all(int(torch.count_nonzero(g)) == 0 for g in zero), "an all-zero v_out must give all-zero gradients"


@pytest.mark.gpu
def test_mask_autograd_and_refusals():
    from gspl_amd import ops
    tables, v_out, ref = _case(1)
    dev = [torch.from_numpy(t).to(DEV).requires_grad_(True) for t in tables]
    dev[3] = torch.from_numpy(tables[3]).to(DEV).reshape(1, 16).requires_grad_(True)      # w2 as nn.Linear keeps it
    out = ops.spotless_mask(*dev, out_size=(17, 19))
    (out * torch.from_numpy(v_out).to(DEV)).sum().backward()
    assert tuple(dev[3].grad.shape) == (1, 16) and tuple(dev[4].grad.shape) == (1,)
    _check_gradients((dev[0].grad.cpu().numpy(), dev[1].grad.cpu().numpy(), dev[2].grad.cpu().numpy(),
                      np.concatenate([dev[3].grad.cpu().numpy().reshape(-1), dev[4].grad.cpu().numpy()])), ref, _chains(tables, (17, 19)))
    G, A, B, w2, b2 = (torch.from_numpy(t).to(DEV) for t in tables)
    same = ops.spotless_mask(G, A, B, w2, b2, out_size=(13, 11))                             # the identity resampling
    assert torch.equal(same, ops.spotless_mask(G, A, B, w2, b2))
    with pytest.raises(NotImplementedError, match="hidden width"):
        ops.spotless_mask(torch.zeros(5, 7, 32, device=DEV), torch.zeros(13, 32, device=DEV), torch.zeros(11, 32, device=DEV),
                          torch.zeros(32, device=DEV), b2)
    with pytest.raises(ValueError, match="at least 2"):
        ops.spotless_mask(G[:1], A, B, w2, b2)
    with pytest.raises(ValueError, match="at least 2"):
        ops.spotless_mask(G, A, B, w2, b2, out_size=(1, 19))
    with pytest.raises(ValueError, match="aligned to 16 bytes"):
        ops.spotless_mask(G, torch.zeros(13 * 16 + 1, device=DEV)[1:].view(13, 16), B, w2, b2)
    with pytest.raises(NotImplementedError, match="float32"):
        ops.spotless_mask(G.double(), A, B, w2, b2)
    transposed = G.permute(1, 0, 2).contiguous().permute(1, 0, 2)                           # not contiguous: copied, as hexplane_encode does
    assert not transposed.is_contiguous() and torch.equal(ops.spotless_mask(transposed, A, B, w2, b2), ops.spotless_mask(G, A, B, w2, b2))


def _frame(H, W, seed, lower, upper):
    """render, gt with: errors exactly equal to either threshold, exactly 0 and exactly 1, render values above 1 (their error leaves the
    histogram's range), and inliers arranged around outliers at a corner and on an edge of the zero padding."""
    rng = np.random.default_rng(seed)
    gt = rng.random((3, H, W), dtype=np.float32)
    render = (gt + (rng.standard_normal((3, H, W)) * 0.4 * (rng.random((1, H, W)) > 0.4)).astype(np.float32)).astype(np.float32)

    def put(y, x, value):
        gt[:, y, x] = 0
        render[:, y, x] = value                              # err = (3 value) / 3: exact for the values used here
    put(5, 5, lower), put(5, 7, upper), put(7, 5, 0.0), put(7, 7, 1.0), put(9, 5, 1.5), put(9, 7, 2.0)
    for (y, x) in ((0, 0), (H - 1, W - 1)):                  # an outlier in a corner: its three neighbours cannot outvote the padding
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if 0 <= y + dy < H and 0 <= x + dx < W:
                    put(y + dy, x + dx, 0.0)
        put(y, x, 1.0)
    for dy in (0, 1):                                        # an outlier on the top edge with five inlier neighbours: voted in
        for dx in (-1, 0, 1):
            put(dy, 9 + dx, 0.0)
    put(0, 9, 1.0)
    for dx in (-1, 0, 1):                                    # ... and on the bottom edge with three: not voted in
        put(H - 1, 13 + dx, 0.0)
    put(H - 2, 12, 0.0), put(H - 2, 13, 1.0), put(H - 2, 14, 1.0), put(H - 1, 13, 1.0)
    return render, gt


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,bins", [(17, 19, 50), (33, 70, 10000)])
def test_error_stats(H, W, bins):
    from gspl_amd import ops
    lower, upper = 0.25, 0.5
    render, gt = _frame(H, W, 7 + H, lower, upper)
    thresholds = torch.tensor([lower, upper], dtype=torch.float32, device=DEV)
    err, counts, lower_mask, upper_mask = (t.cpu().numpy() for t in
                                           ops.spotless_error_stats(torch.from_numpy(render).to(DEV), torch.from_numpy(gt).to(DEV), thresholds, bins))
    want = SO.error_map(render, gt)
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    assert (np.abs(err.astype(np.float64) - want) <= 2 * ulp).all(), "err is more than 2 ulp from the fp64 oracle"
    assert err[5, 5] == np.float32(lower) and err[5, 7] == np.float32(upper) and err[7, 5] == 0 and err[7, 7] == 1 and err[9, 5] == 1.5
    assert counts.dtype == np.int32 and np.array_equal(counts, SO.histogram(err, bins).astype(np.int32))
    in_range = int(((err >= 0) & (err <= 1)).sum())
    assert int(counts.sum()) == in_range and in_range <= H * W - 2
    assert counts[-1] >= 1 and counts[0] >= 1                                  # 1.0 sits in the last bin, 0.0 in the first
    assert np.array_equal(lower_mask, SO.robust_mask(err, np.float32(lower))) and np.array_equal(upper_mask, SO.robust_mask(err, np.float32(upper)))
    assert lower_mask[0, 0] == 0 and upper_mask[0, 0] == 0 and lower_mask[H - 1, W - 1] == 0          # corner outliers stay out
    assert lower_mask[0, 9] == 1 and lower_mask[H - 1, 13] == 0                                        # five neighbours vote in, three do not
    assert 0 < lower_mask.sum() < upper_mask.sum() < H * W


@pytest.mark.gpu
def test_error_stats_threshold_is_strict():
    """A frame whose every error equals the lower threshold exactly: no pixel is an inlier of it, every pixel one of the upper."""
    from gspl_amd import ops
    H, W = 17, 19
    render, gt = np.full((3, H, W), 0.25, dtype=np.float32), np.zeros((3, H, W), dtype=np.float32)
    thresholds = torch.tensor([0.25, 0.5], dtype=torch.float32, device=DEV)
    err, counts, lower_mask, upper_mask = ops.spotless_error_stats(torch.from_numpy(render).to(DEV), torch.from_numpy(gt).to(DEV), thresholds, 50)
    assert bool((err == 0.25).all()) and not bool(lower_mask.any()) and bool((upper_mask == 1).all())
    assert np.array_equal(counts.cpu().numpy(), SO.histogram(err.cpu().numpy(), 50).astype(np.int32))


L1_ROUNDINGS = 4 + (8 + 6 + 3) + (1 + 6 + 3) + 1      # a term: r - g, two additions, the fmaf with the mask; the lane's chain of 8, the butterfly
#                                                       and the four waves; the same in the final kernel (at most 256 partials here); the division


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(17, 19), (33, 70)])      # one partial, and more than one (2048 pixels each)
def test_masked_l1(H, W):
    from gspl_amd import ops
    rng = np.random.default_rng(H)
    gt = rng.random((3, H, W), dtype=np.float32)
    render = (gt + rng.standard_normal((3, H, W)).astype(np.float32) * 0.3).astype(np.float32)
    render[:, 3, 4] = gt[:, 3, 4]                           # equality: sign(0) = 0
    render[1, 5, 6] = gt[1, 5, 6]
    mask = (rng.random((H, W)) > 0.3).astype(np.float32) * rng.random((H, W), dtype=np.float32)
    mask[3, 4] = mask[5, 6] = 0.75
    r = torch.from_numpy(render).to(DEV).requires_grad_(True)
    g, m = torch.from_numpy(gt).to(DEV).requires_grad_(True), torch.from_numpy(mask).to(DEV)[None].requires_grad_(True)
    value = ops.spotless_masked_l1(r, g, m)
    assert value.dim() == 0
    scale = 0.8                                             # (1 - lambda_dssim) in front of the loss
    (scale * value).backward()
    want, want_grad = SO.masked_l1(render, gt, mask, np.float32(scale))
    got_value = float(value.detach())
    print(f"masked l1: |diff| / bound = {abs(got_value - want) / (L1_ROUNDINGS * EPS * want):.3f}")
    assert abs(got_value - want) <= L1_ROUNDINGS * EPS * want
    assert g.grad is None and m.grad is None
    got = r.grad.cpu().numpy()
    assert np.array_equal(np.sign(got), np.sign(want_grad)), "the gradient's sign (0 at equality) differs"
    assert (got[:, 3, 4] == 0).all() and got[1, 5, 6] == 0 and got[0, 5, 6] != 0
    ulp = np.spacing(np.abs(want_grad).astype(np.float32)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - want_grad) <= ulp).all(), "the gradient's magnitude is more than 1 ulp off"


@pytest.mark.gpu
def test_launch_wrappers_refuse_wrong_buffers():
    """The launches alone make the checks of the public ops: a buffer of the wrong size never reaches a kernel."""
    from gspl_amd import ops
    r, g, m = torch.rand(3, 6, 7, device=DEV), torch.rand(3, 6, 7, device=DEV), torch.rand(6, 7, device=DEV)
    one = torch.ones(1, device=DEV)
    for bad in ((r, g[:, :5], m), (r, g, m[:5]), (r, g.double(), m), (r, g.cpu(), m)):
        with pytest.raises((ValueError, NotImplementedError, RuntimeError)):
            ops.spotless_masked_l1_forward(*bad)
        with pytest.raises((ValueError, NotImplementedError, RuntimeError)):
            ops.spotless_masked_l1_backward(*bad, one)
    with pytest.raises(ValueError, match="out must be"):
        ops.spotless_masked_l1_forward(r, g, m, out=torch.empty(0, device=DEV))
    with pytest.raises(ValueError, match="v_render must be"):
        ops.spotless_masked_l1_backward(r, g, m, one, v_render=torch.empty(3, 6, 6, device=DEV))
    with pytest.raises(ValueError, match="grad_out must be"):
        ops.spotless_masked_l1_backward(r, g, m, torch.empty(0, device=DEV))
    tables, v_out, _ = _case(0)
    G, A, B, w2, b2 = (torch.from_numpy(t).to(DEV) for t in tables)
    with pytest.raises(ValueError, match="aligned to 16 bytes"):
        ops.spotless_mask_forward(G, torch.zeros(13 * 16 + 1, device=DEV)[1:].view(13, 16), B, w2, b2)
    with pytest.raises(ValueError, match="v_out must be"):
        ops.spotless_mask_backward(G, A, B, w2, b2, torch.zeros(13, 10, device=DEV))
    with pytest.raises(ValueError, match="v_A must be"):
        ops.spotless_mask_backward(G, A, B, w2, b2, torch.from_numpy(v_out).to(DEV), v_A=torch.empty(12, 16, device=DEV))

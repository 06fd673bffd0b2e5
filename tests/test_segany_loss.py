"""The SegAnyGS ops (include/gspl_hip.h section 24, csrc/segany.hip, ops/segany.py) against the fp64 oracle tests/segany_loss_oracle.py,
which tests/test_segany_loss_cpu.py pins to the reference's own run.

Stages 1 and 2 are integers: bit-exact.  mean_size has two roundings (the exact numerator's conversion and the division).

Stage 3.  eps32 = 2^-23 (one ulp of 1.0; a rounded operation errs by at most half of it, so every count below has the factor 2 of room
that tests/test_spotless.py documents).  The oracle forms the resampling's indices and weights and the pair weight in float32 exactly
as the kernels do, so they carry no error of their own (the weight is asserted bit-equal), and it returns with every sum the sum of the
absolute terms it is made of.
  F         a sample passes 4 rounded operations (two column combines of a product and an fmaf, the row combine the same):
            |F - ref| <= 4 eps32 F_abs.
  corr      |corr| <= 1 and the sum of its absolute terms is <= 1.  An element of X carries the sample's 4 roundings amplified by
            kappa = ||F_abs g|| / ||F g|| (1 where the map is not resampled), the gate product, the C fmaf of the squared norm (halved by
            the root), the root and the division; the chain adds C fmaf:  |corr - ref| <= (C + 8 + 8 kappa) eps32 = R_CORR eps32.
            The oracle's fragile band, 2 (C + 8) eps32, is the issue's.
  loss      a term w label corr / (Ns |M|) carries corr's error, the sum over the scales (Ns), the product with w, the block sum (a
            butterfly of 6 and 3 additions), the cast of the float64 total and the division: (R_CORR + Ns + 12) eps32 loss_abs, loss_abs
            counting |corr| as 1.  The cosines: the same count on a mean of values <= 1.
  v_F       k_n(h, j) has 3 roundings (Ns |M|, the division, the product with w); X_n[j] about C / 2 + 4 + 4 kappa; the chain over j is
            S fmaf; the projection (X . dX, C fmaf; the product and the difference), the division by a norm of C / 2 + 2 roundings, and
            the Ns fmaf with the gates: R_GRAD = S + 2 C + Ns + 8 kappa + 16, times the oracle's absolute sum, plus the terms of the
            pairs whose relu may take the other slope (`*_fragile`).
  v_gates   R_GRAD + the lanes' chains of ceil(S / 64), the butterfly's 6 and the product with F.
  v_rendered R_GRAD + the two weight products and the additions of the samples that share a texel (counted from the indices).
For every non-fragile pair `selected` must equal the oracle's own decision; the fragile pairs are locked to the kernel's decision before
values are compared.  Two runs give the same bits in everything but v_rendered, whose scatter uses float atomics (compared to the same
bound instead).  The GPU tests never widen any of this."""
import functools

import numpy as np
import pytest
import torch

import segany_loss_oracle as SG
from hip_helpers import check_guard_bands, guard_library_blocks
from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)

DEV = "cuda:0"
EPS = SG.EPS32
GRAD_OUT = 0.75


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _within(got, ref, bound, what):
    diff = np.atleast_1d(np.abs(np.asarray(got, dtype=np.float64) - ref))
    bound = np.broadcast_to(bound, diff.shape)
    print(f"{what}: worst |diff| {diff.max():.3e}, worst |diff| / bound = {(diff / np.maximum(bound, 1e-300)).max():.3f}")
    worst = np.unravel_index(np.argmax(diff - bound), diff.shape)
    assert (diff <= bound).all(), f"{what}: |diff| {diff[worst]:.3e} > bound {bound[worst]:.3e} at {worst}"


# ---- stages 1 and 2 ------------------------------------------------------------------------------------------------------------------
#            N_masks  S   image
STAT_CASES = [(1, 1, (1, 1)), (2, 2, (13, 11)), (63, 3, (13, 11)), (64, 64, (13, 11)), (65, 65, (70, 90)), (130, 130, (70, 90))]


@pytest.mark.gpu
@pytest.mark.parametrize("N,S,hw", STAT_CASES)
def test_mask_statistics_and_pair_labels_are_exact(N, S, hw):
    from gspl_amd import ops
    H, W = hw
    masks, scales = SG.random_masks(N, H, W, seed=N)
    rng = np.random.default_rng(100 + N)
    pixel_index = np.sort(rng.choice(H * W, size=S, replace=False)).astype(np.int32)
    order = np.argsort(-scales, kind="stable").astype(np.int32)
    scale_index, upper = SG.scale_picks(N, 10, rng)
    assert scale_index[0] == -1 and scale_index[-1] == N - 1 and 0 in scale_index[1:]

    area_ref, cover_ref, mean_ref, mean_bound = SG.mask_stats(masks)
    member, words = SG.membership(masks, order, pixel_index)
    _, labels_ref, counts_ref = SG.pair_labels(member, scale_index, upper)

    m = _dev(masks)
    for view in (m, m.bool()):
        area, cover, mean_size = ops.segany_mask_stats(view, _dev(order))
        assert area.dtype == torch.int32 and np.array_equal(area.cpu().numpy(), area_ref)
        assert cover.dtype == torch.int32 and np.array_equal(cover.cpu().numpy(), cover_ref)
        _within(mean_size.cpu().numpy(), mean_ref, mean_bound, "mean_size")
    bits = ops.segany_pack_membership(m, _dev(order), _dev(pixel_index))
    assert bits.dtype == torch.int64 and tuple(bits.shape) == (S, (N + 63) // 64) and np.array_equal(bits.cpu().numpy(), words)
    labels, counts = ops.segany_pair_labels(bits, _dev(scale_index), _dev(upper), n_masks=N)
    assert labels.dtype == torch.uint16 and np.array_equal(labels.cpu().numpy(), labels_ref)
    assert np.array_equal(counts.cpu().numpy(), counts_ref) and int(counts.sum()) == S * S
    if N >= 63:
        assert len(set(labels_ref.reshape(-1).tolist())) > 2      # more than the two consistent patterns


# ---- stage 3 -------------------------------------------------------------------------------------------------------------------------
def _golden_case():
    g, inp = SG.golden(), SG.golden_inputs()
    _, labels, counts = SG.pair_labels(inp["member"], inp["scale_index"], inp["upper"])
    return dict(rendered=g["rendered"].astype(np.float32), mask_hw=tuple(g["masks"].shape[1:]), pixel_index=inp["pixel_index"],
                gates=g["gates"].astype(np.float32), labels=labels, counts=counts.astype(np.int32), a=inp["a"], rand=g["draw_rand_ss"])


def _zero_row_case():
    case = SG.make_case(65, 32, 10, "randn", seed=21)
    p = int(case["pixel_index"][7])
    case["rendered"][:, p // case["mask_hw"][1], p % case["mask_hw"][1]] = 0
    return case


def _no_positive_case():
    case = SG.make_case(65, 32, 10, "centres", seed=22)
    case["counts"] = np.array([case["counts"][0], 0, case["counts"][2]], dtype=np.int32)
    return case


def _equal_sizes_case():
    case = SG.make_case(65, 32, 10, "randn", seed=23)
    case["a"][:] = 37.5
    return case


CASES = {
    "golden": _golden_case,
    "randn-300": lambda: SG.make_case(300, 32, 10, "randn", seed=1),
    "centres-300": lambda: SG.make_case(300, 32, 10, "centres", seed=2),
    "randn-65-c4-ns3": lambda: SG.make_case(65, 4, 3, "randn", seed=3),
    "centres-130-c64": lambda: SG.make_case(130, 64, 10, "centres", seed=4),
    "one-pixel": lambda: SG.make_case(1, 32, 10, "randn", seed=5, mask_hw=(3, 3)),
    "two-pixels": lambda: SG.make_case(2, 32, 10, "centres", seed=6, mask_hw=(3, 3)),
    "zero-row": _zero_row_case,
    "no-positive": _no_positive_case,
    "equal-sizes": _equal_sizes_case,
    "upsampled": lambda: SG.make_case(65, 32, 10, "centres", seed=7, mask_hw=(13, 11), render_hw=(7, 5)),
    "downsampled": lambda: SG.make_case(65, 32, 10, "randn", seed=8, mask_hw=(13, 11), render_hw=(20, 24)),
    "downsampled-one-axis": lambda: SG.make_case(65, 32, 3, "centres", seed=9, mask_hw=(13, 11), render_hw=(13, 24)),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    case = CASES[name]()
    return case, SG.loss_of(case)


def _run(case, with_weight=False):
    from gspl_amd import ops
    rendered, gates = _dev(case["rendered"]), _dev(case["gates"])
    args = (_dev(case["pixel_index"]), gates, _dev(case["labels"]), _dev(case["counts"]), _dev(case["a"]), _dev(case["rand"]))
    state = ops.segany_loss_forward(rendered, case["mask_hw"], *args, with_weight=with_weight)
    grads = ops.segany_loss_backward(state, rendered.shape, case["mask_hw"], args[0], gates, args[2], args[4],
                                     torch.tensor([GRAD_OUT], dtype=torch.float32, device=DEV))
    return state, grads


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_loss_forward_and_backward_meet_the_counted_bounds(name):
    case, free = _case(name)
    C, S, Ns = case["rendered"].shape[0], len(case["pixel_index"]), case["gates"].shape[0]
    state, (v_F, v_gates, v_rendered) = _run(case, with_weight=True)
    again, (v_F2, v_gates2, v_rendered2) = _run(case)
    selected = state.selected.cpu().numpy()
    out = state.out.cpu().numpy()

    weight = state.weight.cpu().numpy()
    assert np.array_equal(weight, free["weight"], equal_nan=True), "the in-kernel pair weight is not bit-equal to the float32 matrix"
    _within(state.F.cpu().numpy(), free["F"], 4 * EPS * free["F_abs"], "F")
    firm = ~free["fragile"]
    assert np.array_equal(selected[firm], free["own"][firm]), f"{int((selected[firm] != free['own'][firm]).sum())} non-fragile pairs selected differently"
    assert not selected[np.tril(np.ones((S, S), dtype=bool))].any()

    ref = SG.loss_of(case, lock=selected, grad_out=GRAD_OUT)
    assert state.sel_counts.cpu().numpy().tolist() == [ref["n_pos"], ref["n_neg"]]
    r_corr = C + 8 + 8 * ref["kappa"]
    for k, key in enumerate(("loss", "cosine_pos", "cosine_neg")):
        if np.isnan(ref[key]):
            assert np.isnan(out[k]), f"{key}: the oracle gives NaN, the kernel {out[k]}"
        else:
            _within(out[k], ref[key], EPS * (r_corr + Ns + 12) * (ref["loss_abs"] if key == "loss" else 1.0), key)
    if name in ("one-pixel", "equal-sizes"):
        assert np.isnan(ref["loss"])
    if name == "one-pixel":
        assert not v_F.any() and not v_gates.any() and not v_rendered.any() and np.isnan(ref["cosine_neg"])
    if np.isfinite(ref["loss"]):
        r_grad = S + 2 * C + Ns + 8 * ref["kappa"] + 16
        _within(v_F.cpu().numpy(), ref["v_F"], EPS * r_grad * ref["v_F_abs"] + ref["v_F_fragile"], "v_F")
        _within(v_gates.cpu().numpy(), ref["v_gates"], EPS * (r_grad + -(-S // 64) + 7) * ref["v_gates_abs"] + ref["v_gates_fragile"], "v_gates")
        bound = EPS * (r_grad + 3 + ref["texel_sharing"]) * ref["v_rendered_abs"] + ref["v_rendered_fragile"]
        _within(v_rendered.cpu().numpy(), ref["v_rendered"], bound, "v_rendered")
        _within(v_rendered2.cpu().numpy(), ref["v_rendered"], bound, "v_rendered (second run)")
        if S > 1:
            assert np.abs(ref["v_F"]).max() > 0 and np.abs(ref["v_gates"]).max() > 0

    same = lambda a, b: np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))
    assert same(state.out, again.out) and same(state.selected, again.selected) and same(state.F, again.F), "two forward runs differ in their bits"
    assert same(v_F, v_F2) and same(v_gates, v_gates2), "two backward runs differ in their bits"


@pytest.mark.gpu
def test_hard_sample_branches_fire_both_ways():
    """In the recipe with centres, pairs are selected by each of the three clauses of both sets."""
    case, free = _case("centres-300")
    Ns = case["gates"].shape[0]
    gt = SG.unpack_labels(case["labels"], Ns)
    hard_pos, hard_neg = ((free["corr"] < 0.75) & gt).any(axis=0), ((free["corr"] > 0.5) & ~gt).any(axis=0)
    upper = np.triu(np.ones(hard_pos.shape, dtype=bool), 1)
    total = gt.sum(axis=0)
    assert (hard_pos & upper & (total == Ns)).any() and (hard_neg & upper & (total == 0)).any() and (~hard_neg & upper & (total == 0)).any()
    assert (upper & (total != 0) & (total != Ns)).any()


@pytest.mark.gpu
def test_autograd_reaches_the_map_and_the_gates():
    from gspl_amd import ops
    case, _ = _case("upsampled")
    rendered = _dev(case["rendered"]).requires_grad_(True)
    gates = _dev(case["gates"]).requires_grad_(True)
    args = (_dev(case["pixel_index"]), gates, _dev(case["labels"]), _dev(case["counts"]), _dev(case["a"]), _dev(case["rand"]))
    loss, cosine_pos, cosine_neg, selected = ops.segany_correspondence_loss(rendered, case["mask_hw"], *args, return_selected=True)
    assert loss.dim() == 0 and not cosine_pos.requires_grad and selected.dtype == torch.uint8
    (GRAD_OUT * loss).backward()
    ref = SG.loss_of(case, lock=selected.cpu().numpy(), grad_out=GRAD_OUT)
    C, S, Ns = case["rendered"].shape[0], len(case["pixel_index"]), case["gates"].shape[0]
    r_grad = S + 2 * C + Ns + 8 * ref["kappa"] + 16
    _within(gates.grad.cpu().numpy(), ref["v_gates"], EPS * (r_grad + -(-S // 64) + 7) * ref["v_gates_abs"] + ref["v_gates_fragile"], "v_gates")
    _within(rendered.grad.cpu().numpy(), ref["v_rendered"],
            EPS * (r_grad + 3 + ref["texel_sharing"]) * ref["v_rendered_abs"] + ref["v_rendered_fragile"], "v_rendered")
    fixed = ops.segany_correspondence_loss(rendered, case["mask_hw"], args[0], gates.detach(), *args[2:])      # the fixed gate table: no gradient asked
    assert torch.equal(fixed[0].detach(), loss.detach())
    rendered.grad = None
    fixed[0].backward()
    assert rendered.grad is not None and gates.grad is not None


@pytest.mark.gpu
def test_refusals():
    from gspl_amd import ops
    case, _ = _case("two-pixels")
    rendered, gates = _dev(case["rendered"]), _dev(case["gates"])
    args = [_dev(case["pixel_index"]), gates, _dev(case["labels"]), _dev(case["counts"]), _dev(case["a"]), _dev(case["rand"])]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.segany_correspondence_loss(rendered.cpu(), case["mask_hw"], *args)
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        ops.segany_correspondence_loss(rendered[:30], case["mask_hw"], args[0], gates[:, :30].contiguous(), *args[2:])
    with pytest.raises(NotImplementedError, match="float32"):
        ops.segany_correspondence_loss(rendered.double(), case["mask_hw"], *args)
    with pytest.raises(ValueError, match="labels must be"):
        ops.segany_correspondence_loss(rendered, case["mask_hw"], args[0], gates, args[2][:1], *args[3:])
    with pytest.raises(NotImplementedError, match="masks are built"):
        ops.segany_mask_stats(torch.zeros(1025, 2, 2, dtype=torch.uint8, device=DEV))
    with pytest.raises(NotImplementedError, match="uint8"):
        ops.segany_mask_stats(torch.zeros(2, 2, 2, device=DEV))
    with pytest.raises(NotImplementedError, match="S <= 4096"):
        ops.segany_pack_membership(torch.zeros(2, 80, 80, dtype=torch.uint8, device=DEV), torch.arange(2, device=DEV), torch.arange(4097, device=DEV))
    with pytest.raises(NotImplementedError, match="Ns <= 16"):
        ops.segany_pair_labels(torch.zeros(3, 1, dtype=torch.int64, device=DEV), torch.zeros(17, dtype=torch.int32, device=DEV),
                               torch.zeros(17, dtype=torch.uint8, device=DEV))
    from gspl_amd import _lib as L
    assert L.lib().gspl_segany_pair_labels(4097, 1, 1, None, None, None, None, None, None, None) == L.GSPL_ERR_INVALID_ARG
    assert L.lib().gspl_segany_loss_fwd(2, 6, 1, 2, 2, 2, 2, *([None] * 13), 0, None) == L.GSPL_ERR_INVALID_ARG
    assert L.lib().gspl_segany_loss_workspace_bytes(2, 32, 17) == 0


@pytest.mark.gpu
def test_scratch_blocks_keep_their_guard_bands(monkeypatch):
    """Every scratch block of the new ops (the packed membership words, the heads, the loss workspace) between two poisoned bands."""
    from gspl_amd import ops
    outers = guard_library_blocks(monkeypatch)
    masks, scales = SG.random_masks(65, 70, 90, seed=65)
    m, order = _dev(masks), _dev(np.argsort(-scales, kind="stable").astype(np.int32))
    pixel_index = _dev(np.arange(0, 70 * 90, 97, dtype=np.int32))
    ops.segany_mask_stats(m, order)
    bits = ops.segany_pack_membership(m, order, pixel_index)
    rng = np.random.default_rng(0)
    scale_index, upper = SG.scale_picks(65, 10, rng)
    ops.segany_pair_labels(bits, _dev(scale_index), _dev(upper), n_masks=65)
    _run(_case("randn-65-c4-ns3")[0])
    _run(_case("centres-130-c64")[0])
    assert check_guard_bands(outers, "segany ops") >= 6

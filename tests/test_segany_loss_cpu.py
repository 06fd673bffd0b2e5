"""The fp64 oracle tests/segany_loss_oracle.py against the reference's own run (tests/golden/ref_segany_loss.npz, written by
tests/golden/make_segany_loss_golden.py), the condition that keeps the GPU tests' locked selection honest, and the header's new
entry points.  No GPU."""
import re

import numpy as np

import segany_loss_oracle as SG

ENTRY_POINTS = ("gspl_segany_mask_stats", "gspl_segany_pack_membership", "gspl_segany_pair_labels", "gspl_segany_loss_fwd", "gspl_segany_loss_bwd")


golden, golden_inputs = SG.golden, SG.golden_inputs


def test_sampled_pixels_follow_the_recorded_draw():
    g = golden()
    _, cover, _, _ = SG.mask_stats(g["masks"])
    assert np.array_equal(g["sampled_ray"], (g["draw_rand_hw"] < np.float32(g["ray_sample_rate"])) & (cover > 0))
    assert (cover == 0).any() and g["sampled_ray"].sum() >= 25


def test_labels_and_counts_equal_the_reference_loop():
    g, inp = golden(), golden_inputs()
    gt, labels, counts = SG.pair_labels(inp["member"], inp["scale_index"], inp["upper"])
    assert gt.shape == g["gt_corrs"].shape and np.array_equal(gt, g["gt_corrs"] != 0)
    assert np.array_equal(SG.unpack_labels(labels, 10), gt)
    total = g["gt_corrs"].astype(np.int64).sum(axis=0)
    assert counts.tolist() == [int((total == 0).sum()), int((total == 10).sum()), int(((total != 0) & (total != 10)).sum())]
    assert min(counts) > 0 and inp["upper"].sum() >= 1 and 0 in inp["upper"]


def test_membership_words_hold_the_sorted_bits():
    inp = golden_inputs()
    words = inp["words"].view(np.uint64)
    for i in range(inp["member"].shape[1]):
        assert np.array_equal((words[:, i // 64] >> np.uint64(i % 64)) & np.uint64(1), inp["member"][:, i].astype(np.uint64))


def test_weight_is_bit_equal_to_the_reference_matrix():
    weight = SG.pair_weight(golden_inputs()["a"])
    assert weight.dtype == np.float32 and np.array_equal(weight.view(np.uint32), golden()["per_pixel_weight"].view(np.uint32))
    assert weight.min() == 1 and weight.max() == 10


def _golden_loss():
    g, inp = golden(), golden_inputs()
    _, labels, counts = SG.pair_labels(inp["member"], inp["scale_index"], inp["upper"])
    return SG.loss(g["rendered"], g["masks"].shape[1:], inp["pixel_index"], g["gates"], labels, counts, inp["a"], g["draw_rand_ss"], dtype=np.float64)


def test_loss_cosines_and_gradients_match_the_reference():
    g, ref = golden(), _golden_loss()
    close = lambda got, want: np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)
    assert ref["n_pos"] > 0 and ref["n_neg"] > 0
    for name in ("loss", "cosine_pos", "cosine_neg"):
        assert close(np.float64(ref[name]), g[name]), name
    assert close(ref["v_rendered"], g["grad_rendered"]) and close(ref["v_gates"], g["grad_gates"])
    slope = g["gates"] * (1 - g["gates"])                      # through the sigmoid and the Linear(1, C) by hand
    assert close((ref["v_gates"] * slope * g["sampled_scales"][:, None]).sum(axis=0), g["grad_gate_weight"][:, 0])
    assert close((ref["v_gates"] * slope).sum(axis=0), g["grad_gate_bias"])
    assert (np.abs(ref["v_F"]) <= ref["v_F_abs"] * (1 + 1e-12)).all() and (np.abs(ref["v_gates"]) <= ref["v_gates_abs"] * (1 + 1e-12)).all()
    assert (np.abs(ref["v_rendered"]) <= ref["v_rendered_abs"] * (1 + 1e-12)).all()


def test_lock_moves_only_fragile_pairs():
    g, inp = golden(), golden_inputs()
    _, labels, counts = SG.pair_labels(inp["member"], inp["scale_index"], inp["upper"])
    args = (g["rendered"], g["masks"].shape[1:], inp["pixel_index"], g["gates"], labels, counts, inp["a"], g["draw_rand_ss"])
    free = SG.loss(*args)
    flipped = SG.loss(*args, lock=free["own"] ^ 3)
    assert np.array_equal(flipped["selected"][~free["fragile"]], free["own"][~free["fragile"]])
    assert np.array_equal(flipped["selected"][free["fragile"]], (free["own"] ^ 3)[free["fragile"]])


RECIPES = ("randn", "centres")


def test_fragile_pairs_are_rare():
    """For each input recipe of the GPU tests, at S = 600, C = 32 and 10 sigmoid(randn) gates: the fragile pairs are at most 1e-3 of
    the pairs.  A condition, not a measurement: it keeps the locked selection from hiding a wrong kernel."""
    for recipe in RECIPES:
        ref = SG.loss_of(SG.make_case(600, 32, 10, recipe, seed=11))
        pairs = 600 * 599 // 2
        fragile = int(ref["fragile"].sum())
        high = float((ref["corr"][:, np.triu(np.ones((600, 600), dtype=bool), 1)] > 0.75).any(axis=0).mean())
        print(f"{recipe}: {fragile} fragile of {pairs} pairs ({fragile / pairs:.2e}); pairs above 0.75 at some scale: {high:.3f}")
        assert fragile <= 1e-3 * pairs
        if recipe == "centres":
            assert high > 0.03
        assert ref["n_pos"] > 0 and ref["n_neg"] > 0 and ref["kappa"] < 1 + 1e-9


def test_header_declares_the_entry_points_and_the_binding_finds_them():
    from gspl_amd import _lib
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    assert re.search(r"#define\s+GSPL_ABI_VERSION\s+39\b", text) and _lib.ABI_VERSION == 39
    assert "24. The SegAnyGS" in text and "PURELY ADDITIVE" in text[text.index("24. The SegAnyGS"):]
    for name in ENTRY_POINTS:
        assert f"int {name}(" in text and name in _lib.exported_symbols()
    assert "size_t gspl_segany_loss_workspace_bytes(" in text and "gspl_segany_loss_workspace_bytes" in _lib.exported_symbols()

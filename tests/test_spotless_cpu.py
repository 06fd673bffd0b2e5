"""The SpotLess route without a GPU: the oracle tests/spotless_oracle.py, the cached positional encoding, the fold
(`gspl_amd.spotless.predict_mask_torch`) and `RunningErrorStats` against tests/golden/ref_spotless.npz, which
tests/golden/make_spotless_golden.py wrote from the reference's own `SpotLessMetricsModule`."""
import os
import types

import numpy as np
import pytest
import torch

import spotless_oracle as SO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_spotless.npz")
H, W = 13, 11
BRANCHES = [("", 800, None, "pe32"), ("_r", 9, (H, W), "pe32_9")]


@pytest.fixture(scope="module")
def ref():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _state(ref):
    return {k[len("state/"):]: v for k, v in ref.items() if k.startswith("state/")}


def _module(ref, dtype):
    """An object with the reference's `mlp.0` / `mlp.2` layers, nothing else of it."""
    state = _state(ref)
    mlp = torch.nn.Sequential(torch.nn.Linear(state["mlp.0.weight"].shape[1], 16), torch.nn.ReLU(), torch.nn.Linear(16, 1), torch.nn.Sigmoid())
    module = types.SimpleNamespace(mlp=mlp.to(dtype))
    mlp.load_state_dict({k[len("mlp."):]: torch.from_numpy(v).to(dtype) for k, v in state.items()})
    return module


@pytest.mark.parametrize("tag,size,out_size,pe", BRANCHES)
def test_oracle_matches_the_reference(ref, tag, size, out_size, pe):
    """The oracle on the folded tables, weights formed in float64 as torch forms them for float64 input: mask, spot loss, regulariser and
    the four parameter gradients (the oracle's table gradients carried through the fold's three products) within 1e-12."""
    state = _state(ref)
    G, A, B, w2, b2 = SO.fold(state, ref["sf"], ref[pe])
    fwd = SO.mask(G, A, B, w2, b2, out_size, dtype=np.float64)
    assert np.abs(fwd["out"] - ref["mask64" + tag].reshape(H, W)).max() <= 1e-12
    assert np.abs(fwd["out"].reshape(ref["up64" + tag].shape) - ref["up64" + tag]).max() <= 1e-12
    assert abs(SO.spot_loss(fwd["out"], ref["upper_mask"], ref["lower_mask"]) - float(ref["spot64" + tag])) <= 1e-12
    assert abs(0.5 * SO.regulariser(state["mlp.0.weight"], state["mlp.2.weight"]) - float(ref["reg64" + tag])) <= 1e-12
    v_out = SO.spot_loss_grad(fwd["out"], ref["upper_mask"].reshape(H, W), ref["lower_mask"].reshape(H, W))
    assert np.abs(v_out).sum() > 0
    res = SO.mask(G, A, B, w2, b2, out_size, v_out, dtype=np.float64)
    C, sf, enc = ref["sf"].shape[0], ref["sf"].astype(np.float64), ref[pe].astype(np.float64)
    v_W1 = np.concatenate([np.einsum("yxk,cyx->kc", res["v_G"], sf), res["v_A"].T @ enc[:, 0, :40], res["v_B"].T @ enc[0, :, 40:]], axis=1)
    for name, got in (("mlp.0.weight", v_W1), ("mlp.0.bias", res["v_A"].sum(axis=0)), ("mlp.2.weight", res["v_w2"][None]), ("mlp.2.bias", res["v_b2"])):
        assert np.abs(got - ref["grad64" + tag + "/" + name]).max() <= 1e-12, name
    assert C == 24 and v_W1.shape == state["mlp.0.weight"].shape


@pytest.mark.parametrize("I,O", [(5, 13), (7, 11), (13, 17), (11, 19), (13, 12), (11, 5), (2, 3), (50, 70), (50, 90), (70, 100), (90, 61), (9, 13)])
def test_oracle_float32_resampling_rule_is_torchs(I, O):
    """The oracle's float32 indices and weights against F.interpolate itself, independent of any kernel: a one-hot input per source
    row reads the weight of that row out exactly (weight x 1 + weight x 0), for every axis pair the GPU tests resample."""
    import torch.nn.functional as F
    onehot = torch.eye(I, dtype=torch.float32).reshape(1, I, I, 1).expand(1, I, I, 2).contiguous()      # channel c: 1 on row c
    got = F.interpolate(onehot, size=(O, 2), mode="bilinear")[0, :, :, 0].t().numpy()                  # [O, I]
    assert np.array_equal(SO.resample_matrix(I, O, np.float32).astype(np.float32), got)
    ramp = torch.arange(I, dtype=torch.float32).reshape(1, 1, I, 1).expand(1, 1, I, 2).contiguous()
    want = F.interpolate(ramp, size=(O, 2), mode="bilinear")[0, 0, :, 0].numpy().astype(np.float64)
    assert np.abs(SO.resample_matrix(I, O, np.float32) @ np.arange(I, dtype=np.float64) - want).max() <= 2 * I * SO.EPS32


def test_oracle_robust_mask_and_running_stats_match_the_reference(ref):
    err = ref["err_map"][0].mean(axis=-1)                                           # float32, as `robust_mask` forms it
    err_t = torch.from_numpy(ref["err_map"]).mean(axis=-1)[0].numpy()
    for thr, want in ((float(ref["thr_a"]), ref["robust_a"]), (float(ref["thr_b"]), ref["robust_b"])):
        assert np.array_equal(SO.robust_mask(err_t, thr), want.reshape(H, W))
        assert 0 < want.sum() < want.size
    assert np.abs(err - err_t).max() <= 1e-7
    frame = SO.error_map(ref["render"], ref["gt"]).astype(np.float32)
    assert np.array_equal(SO.robust_mask(frame, float(ref["lower_thr"])), ref["lower_mask"].reshape(H, W))
    assert np.array_equal(SO.robust_mask(frame, float(ref["upper_thr"])), ref["upper_mask"].reshape(H, W))
    hist = np.zeros(50, dtype=np.float32)
    for step in range(3):
        counts = SO.histogram(SO.error_map(ref["stats_render"][step], ref["stats_gt"][step]), 50)
        assert np.array_equal(counts, ref["stats_counts"][step])
        hist, (avg, lower, upper) = SO.running_stats(hist, counts, 50, (0.7, 0.5, 0.9))
        assert np.abs(hist - ref["stats_hist"][step]).max() <= 1e-6
        assert (avg, lower, upper) == (ref["stats_avg"][step], ref["stats_lower"][step], ref["stats_upper"][step])


def test_positional_encoding_cache_is_the_references_bit_for_bit(ref):
    import gspl_amd  # noqa: F401
    from gspl_amd import spotless
    for (mh, mw), key in (((13, 11), "pe32"), ((9, 9), "pe32_9")):
        pe_y, pe_x = spotless.positional_encodings(mh, mw, "cpu")
        assert pe_y.dtype == torch.float32 and tuple(pe_y.shape) == (mh, 40) and tuple(pe_x.shape) == (mw, 40)
        assert spotless.positional_encodings(mh, mw, "cpu")[0] is pe_y                     # cached
        want = ref[key]
        # exactly separable: the first 40 channels depend on the row only, the last 40 on the column only
        assert np.array_equal(want[:, :, :40], np.broadcast_to(want[:, :1, :40], want[:, :, :40].shape))
        assert np.array_equal(want[:, :, 40:], np.broadcast_to(want[:1, :, 40:], want[:, :, 40:].shape))
        assert np.array_equal(pe_y.numpy(), want[:, 0, :40]) and np.array_equal(pe_x.numpy(), want[0, :, 40:])
    with pytest.raises(ValueError, match="at least 2"):
        spotless.positional_encodings(1, 5, "cpu")


@pytest.mark.parametrize("tag,size,out_size,pe", BRANCHES)
def test_fold_in_float64_matches_the_reference(ref, tag, size, out_size, pe):
    import gspl_amd  # noqa: F401
    from gspl_amd import spotless
    module = _module(ref, torch.float64)
    up, mask = spotless.predict_mask_torch(module, torch.from_numpy(ref["sf"]).double(), H, W, size)
    assert tuple(up.shape) == ref["up64" + tag].shape and tuple(mask.shape) == ref["mask64" + tag].shape
    assert float((mask.detach() - torch.from_numpy(ref["mask64" + tag])).abs().max()) <= 1e-12
    assert float((up.detach() - torch.from_numpy(ref["up64" + tag])).abs().max()) <= 1e-12
    upper, lower = torch.from_numpy(ref["upper_mask"]).double().flatten(), torch.from_numpy(ref["lower_mask"]).double().flatten()
    spot = torch.mean(torch.relu(up.flatten() - upper) + torch.relu(lower - up.flatten()))
    assert abs(float(spot.detach()) - float(ref["spot64" + tag])) <= 1e-12
    spot.backward()
    for name, p in module.mlp.named_parameters():
        assert float((p.grad - torch.from_numpy(ref["grad64" + tag + "/mlp." + name])).abs().max()) <= 1e-12, name


@pytest.mark.parametrize("tag,size,out_size,pe", BRANCHES)
def test_fold_in_float32_is_as_close_as_the_references_own_float32_run(ref, tag, size, out_size, pe):
    """The largest error of the folded float32 form against the float64 reference may not exceed 4 x the largest error of the
    reference's own float32 run, plus 1 ulp of 1.0: the factor covers the other summation order of a 104-term product, nothing else."""
    import gspl_amd  # noqa: F401
    from gspl_amd import spotless
    with torch.no_grad():
        _, mask = spotless.predict_mask_torch(_module(ref, torch.float32), torch.from_numpy(ref["sf"]), H, W, size)
    assert mask.dtype == torch.float32
    ours = np.abs(mask.numpy().astype(np.float64) - ref["mask64" + tag]).max()
    theirs = np.abs(ref["mask32" + tag].astype(np.float64) - ref["mask64" + tag]).max()
    print(f"float32 fold{tag}: ours {ours:.3e}, the reference's own {theirs:.3e}")
    assert ours <= 4 * theirs + SO.EPS32


def test_running_error_stats_follow_the_reference(ref):
    import gspl_amd  # noqa: F401
    from gspl_amd import spotless
    stats = spotless.RunningErrorStats(bins=50, robust_percentile=0.7, lower_bound=0.5, upper_bound=0.9, device="cpu")
    assert float(stats.avg) == 1.0 and float(stats.lower) == 0.0 and float(stats.upper) == 1.0 and not stats.hist.any()
    for step in range(3):
        stats.update(torch.from_numpy(ref["stats_counts"][step]).to(torch.int32))
        assert float((stats.hist - torch.from_numpy(ref["stats_hist"][step])).abs().max()) <= 1e-6
        assert (float(stats.avg), float(stats.lower), float(stats.upper)) == \
               (float(ref["stats_avg"][step]), float(ref["stats_lower"][step]), float(ref["stats_upper"][step]))
    assert tuple(stats.thresholds.shape) == (2,) and float(stats.thresholds[1]) == float(ref["stats_upper"][2])


def test_ops_refuse_the_cpu_and_the_wrong_shapes():
    import gspl_amd  # noqa: F401
    from gspl_amd import ops, spotless
    G, A, B, w2, b2 = torch.zeros(5, 7, 16), torch.zeros(13, 16), torch.zeros(11, 16), torch.zeros(16), torch.zeros(1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.spotless_mask(G, A, B, w2, b2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.spotless_error_stats(torch.zeros(3, 4, 4), torch.zeros(3, 4, 4), torch.zeros(2), 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.spotless_masked_l1(torch.zeros(3, 4, 4), torch.zeros(3, 4, 4), torch.zeros(4, 4))
    placeholder = spotless.HipSpotLessMetrics()
    assert (placeholder.lower_bound, placeholder.upper_bound, placeholder.bin_size, placeholder.max_mlp_mask_size) == (0.5, 0.9, 10000, 800)
    if spotless._SpotLessMetrics is None:
        with pytest.raises(RuntimeError, match="inside the reference repository"):
            placeholder.instantiate()

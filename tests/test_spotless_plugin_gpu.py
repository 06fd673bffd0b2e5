"""The SpotLess plugin's functional core on the GPU (gspl_amd/spotless.py): `predict_mask` against `predict_mask_torch` and a
float64 run of the fold on the device (weights and frame of tests/golden/ref_spotless.npz), a training step's calls without a host wait, and the three ops between
poisoned guard bands (in the style of tests/test_hexplane_lifetime.py)."""
import os
import types

import numpy as np
import pytest
import torch

import spotless_oracle as SO
from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_spotless.npz")
H, W = 13, 11


@pytest.fixture(scope="module")
def ref():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _module(ref, device, dtype=torch.float32):
    mlp = torch.nn.Sequential(torch.nn.Linear(24 + 80, 16), torch.nn.ReLU(), torch.nn.Linear(16, 1), torch.nn.Sigmoid())
    mlp.load_state_dict({k[len("state/mlp."):]: torch.from_numpy(v).float() for k, v in ref.items() if k.startswith("state/")})
    return types.SimpleNamespace(mlp=mlp.to(device=device, dtype=dtype))      # (the float32 weights, widened exactly)


def _spot(up, ref):
    upper, lower = (torch.from_numpy(ref[k]).to(device=up.device, dtype=up.dtype).flatten() for k in ("upper_mask", "lower_mask"))
    return torch.mean(torch.relu(up.flatten() - upper) + torch.relu(lower - up.flatten()))


@pytest.mark.parametrize("tag,size", [("", 800), ("_r", 9)])
def test_predict_mask_against_the_torch_fold_and_a_float64_run(ref, tag, size):
    """`predict_mask` against `predict_mask_torch`, both branches, masks and the gradients of the four parameters.

    The float64 reference is the fold in float64 torch ops ON THIS DEVICE, from the same float32 weights and the same cached float32
    positional encoding (`fold` widens the cache), so it differs from a float32 run by that run's rounding alone.  (The CPU fixture is
    no reference here: this device forms `index / (n - 1)` of the encoding one ulp off the CPU's at 13 x 11.)
      fold criterion   the op's largest error against the float64 run may not exceed 4 x the largest error of the float32 torch fold
                       against it, plus 1 ulp of 1.0; for a parameter's gradient both errors are taken relative to the gradient's largest
                       magnitude, so that `1 ulp of 1.0` means the same there.
      directly         the op and the float32 torch fold evaluate the SAME float32 tables G, A, B, w2, b2 (the fold is the same code),
                       each within the counted forward bound of tests/test_spotless.py of the oracle on those tables (the torch
                       formulation passes no more rounded operations than the count): the op within 1 x that bound of the oracle, the two
                       within 2 x of each other."""
    from gspl_amd import spotless
    sf = torch.from_numpy(ref["sf"]).to(DEV)
    runs = {}
    for name, fn, dtype in (("hip", spotless.predict_mask, torch.float32), ("torch", spotless.predict_mask_torch, torch.float32),
                            ("float64", spotless.predict_mask_torch, torch.float64)):
        module = _module(ref, DEV, dtype)
        up, mask = fn(module, sf.to(dtype), H, W, size)
        assert up.dtype == dtype and tuple(up.shape) == ref["up64" + tag].shape and tuple(mask.shape) == ref["mask64" + tag].shape
        assert torch.equal(up.flatten(), mask.flatten())
        _spot(up, ref).backward()
        runs[name] = (mask.detach().double().cpu().numpy().reshape(H, W), {n: p.grad.double().cpu().numpy() for n, p in module.mlp.named_parameters()})
    want_mask, want_grads = runs["float64"]
    assert all(np.abs(g).max() > 0 for g in want_grads.values())
    errors = {}
    for name in ("hip", "torch"):
        mask, grads = runs[name]
        errors[name] = [np.abs(mask - want_mask).max()] + [np.abs(grads[n] - want_grads[n]).max() / np.abs(want_grads[n]).max() for n in want_grads]
    print(f"predict_mask{tag}: errors (mask, then the four gradients) hip {['%.2e' % e for e in errors['hip']]}, "
          f"torch {['%.2e' % e for e in errors['torch']]}")
    for ours, theirs in zip(errors["hip"], errors["torch"]):
        assert ours <= 4 * theirs + SO.EPS32
    mh, mw = (size, size) if max(H, W) > size else (H, W)
    with torch.no_grad():
        tables = [t.cpu().numpy() for t in spotless.fold(_module(ref, DEV), sf, mh, mw)]
    oracle = SO.mask(*tables, (H, W))
    hip, plain = runs["hip"][0], runs["torch"][0]
    print(f"predict_mask{tag}: |hip - oracle| / bound {(np.abs(hip - oracle['out']) / oracle['out_bound']).max():.3f}, "
          f"|hip - torch| / bound {(np.abs(hip - plain) / oracle['out_bound']).max():.3f}")
    assert (np.abs(hip - oracle["out"]) <= oracle["out_bound"]).all()
    assert (np.abs(hip - plain) <= 2 * oracle["out_bound"]).all()


def test_a_training_step_makes_no_host_wait(ref):
    """`predict_mask`, `spotless_error_stats`, `spotless_masked_l1` (each with its backward) and `RunningErrorStats.update` under
    torch.cuda.set_sync_debug_mode("error").  The caches (positional encoding, histogram edges) are filled by the step before, as
    in training."""
    from gspl_amd import ops, spotless
    module = _module(ref, DEV)
    sf = torch.from_numpy(ref["sf"]).to(DEV)
    render = torch.from_numpy(ref["render"]).to(DEV).requires_grad_(True)
    gt = torch.from_numpy(ref["gt"]).to(DEV)
    stats = spotless.RunningErrorStats(bins=50, device=DEV)

    def step(size):
        _, counts, lower, upper = ops.spotless_error_stats(render, gt, stats.thresholds, stats.bins)
        up, mask = spotless.predict_mask(module, sf, H, W, size)
        loss = ops.spotless_masked_l1(render, gt, mask.squeeze(-1).detach())
        (0.8 * loss).backward()
        torch.mean(torch.relu(up.flatten() - upper.flatten()) + torch.relu(lower.flatten() - up.flatten())).backward()
        stats.update(counts)
        return loss

    step(800), step(9)
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=DEV).item()
            takes_effect = False
        except RuntimeError:
            takes_effect = True
        if takes_effect:
            losses = [step(800), step(9)]
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    if not takes_effect:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not take effect on this build")
    assert all(bool(torch.isfinite(l)) for l in losses) and float(stats.upper) <= 1.0 and bool(stats.hist.sum() > 0)


BAND = 1024          # elements of 4 bytes


def _arena(sizes):
    starts, at = [], BAND
    for n in sizes:
        starts.append(at)
        at += n + (-n) % 4 + BAND                      # keeps the next slot on a 16-byte boundary
    arena = torch.empty((at,), dtype=torch.float32, device=DEV)
    poison = torch.tensor(0x7FC0DEAD, dtype=torch.int32, device=DEV)
    arena.view(torch.int32).fill_(poison)
    return arena, starts, poison


def _run_between_bands(fill_byte):
    from gspl_amd import ops
    (h0, w0), (mh, mw), (OH, OW), bins = (5, 7), (13, 11), (17, 19), 50
    sizes = [OH * OW, h0 * w0 * 16, mh * 16, mw * 16, 17,          # the mask op: out, v_G, v_A, v_B, v_w
             OH * OW, bins, OH * OW, OH * OW,                      # error stats: err, counts, lower, upper
             1, 3 * OH * OW]                                       # masked l1: out, v_render
    arena, starts, poison = _arena(sizes)
    slots = [arena[s:s + n] for s, n in zip(starts, sizes)]
    for slot in slots:
        slot.view(torch.uint8).fill_(fill_byte)
    out, v_G, v_A, v_B, v_w = slots[0].view(OH, OW), slots[1].view(h0, w0, 16), slots[2].view(mh, 16), slots[3].view(mw, 16), slots[4]
    err, counts, lower, upper = slots[5].view(OH, OW), slots[6].view(torch.int32), slots[7].view(OH, OW), slots[8].view(OH, OW)
    l1, v_render = slots[9], slots[10].view(3, OH, OW)
    g = torch.Generator().manual_seed(3)
    G, A, B, w2, b2 = (torch.randn(s, generator=g).to(DEV) for s in ((h0, w0, 16), (mh, 16), (mw, 16), (16,), (1,)))
    gt = torch.rand(3, OH, OW, generator=g).to(DEV)
    render = (gt + 0.3 * torch.randn(3, OH, OW, generator=g).to(DEV)).contiguous()
    ops.spotless_mask_forward(G, A, B, w2, b2, out_size=(OH, OW), out=out)
    ops.spotless_mask_backward(G, A, B, w2, b2, torch.randn(OH, OW, generator=g).to(DEV), (OH, OW), v_G, v_A, v_B, v_w)
    ops.spotless_error_stats(render, gt, torch.tensor([0.1, 0.3], device=DEV), bins, out=(err, counts, lower, upper))
    ops.spotless_masked_l1_forward(render, gt, out.contiguous(), out=l1)
    ops.spotless_masked_l1_backward(render, gt, out.contiguous(), torch.ones(1, device=DEV), v_render=v_render)
    torch.cuda.synchronize()
    words = arena.view(torch.int32)
    edges = [0] + [e for s, n in zip(starts, sizes) for e in (s, s + n)] + [arena.numel()]
    for lo, hi in zip(edges[0::2], edges[1::2]):
        assert bool((words[lo:hi] == poison).all()), f"the band [{lo}, {hi}) was written"
    floats = [s for k, s in enumerate(slots) if k != 6]
    assert all(bool(torch.isfinite(s).all()) for s in floats) and all(bool(s.any()) for s in floats)
    assert int(counts.sum()) == int(((err >= 0) & (err <= 1)).sum()) > 0
    return [s.clone() for s in slots]


def test_guard_bands_stay_intact_and_prefill_does_not_matter():
    a, b = _run_between_bands(0xFF), _run_between_bands(0x00)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))

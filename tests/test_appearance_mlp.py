"""The fused appearance MLP (include/gspl_hip.h section 21, csrc/appearance.hip, ops/appearance.py) against tests/appearance_oracle.py.

Exact tests: integer-valued data whose every intermediate, and the sum of absolute products behind every element of every matrix
product, stays below 2^24 (the oracle computes in int64 and asserts that bound), so exact fp32 arithmetic gives the oracle's bits in
any summation order; every output and every gradient must be EQUAL.  A wrong MFMA lane map therefore fails an equality.
Random parity against the fp64 oracle: forward |got - ref| <= 1e-5, every gradient element <= 1e-4 (|ref| + rms(ref)) of its tensor
(this project's locked parity).  The row counts come from the kernel's constants: T rows of a wave tile, B rows of a workgroup pass,
G workgroups.  The observed maxima are printed (DESIGN.md section 7 records them):
    forward at most 7.3e-8; gradients, as a fraction of their bound, at most 0.029."""
import functools

import pytest
import torch

import appearance_oracle as AO
from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)

DEV = "cuda:0"
gpu = pytest.mark.gpu


def _constants():
    from gspl_amd.ops import appearance as A
    return A.ROW_TILE, A.ROWS_PER_PASS, A.GRID_SIZE


def _row_counts():
    T, B, G = _constants()
    return [0, 1, T - 1, T, T + 1, B - 1, B + 1, G * B + 1]


@functools.lru_cache(maxsize=None)
def _integer_case(N, F, E, H, L, n_out, mask_kind="none"):
    """(inputs, mask, oracle out, oracle gradients) of one exact case; computed once, never modified."""
    features, weights, biases, embedding, v_out = AO.integer_case(N, F, E, H, L, n_out, seed=N + 7 * F + L)
    mask = _mask(mask_kind, N)
    out, grads, bound = AO.exact(features, weights, biases, embedding, v_out, mask=mask)
    return (features, weights, biases, embedding, v_out), mask, out, grads, bound


def _mask(kind, N):
    B = _constants()[1]
    if kind == "none":
        return None
    if kind == "all":
        return torch.ones(N, dtype=torch.bool)
    if kind == "nothing":
        return torch.zeros(N, dtype=torch.bool)
    if kind == "alternating":
        return torch.arange(N) % 2 == 1
    assert kind == "last_of_block"
    mask = torch.zeros(N, dtype=torch.bool)
    mask[B - 1] = True
    return mask


def _run(inputs, mask=None, means=None, camera_center=None, **options):
    """The op and its backward on the GPU -> (out, dict of gradients), on the CPU."""
    from gspl_amd import ops
    features, weights, biases, embedding, v_out = inputs
    leaf = lambda t: t.to(DEV).requires_grad_(True)
    f, e, ws, bs = leaf(features), leaf(embedding), [leaf(w) for w in weights], [leaf(b) for b in biases]
    out = ops.appearance_mlp(f, ws, bs, e, mask=None if mask is None else mask.to(DEV), means=None if means is None else means.to(DEV),
                             camera_center=None if camera_center is None else camera_center.to(DEV), **options)
    out.backward(v_out.to(DEV))
    torch.cuda.synchronize()
    return out.detach().cpu(), dict(v_features=f.grad.cpu(), v_weights=[w.grad.cpu() for w in ws], v_biases=[b.grad.cpu() for b in bs],
                                    v_embedding=e.grad.cpu())


def _tensors(grads):
    return [("v_features", grads["v_features"]), ("v_embedding", grads["v_embedding"])] + \
        [(f"v_weights[{i}]", w) for i, w in enumerate(grads["v_weights"])] + [(f"v_biases[{i}]", b) for i, b in enumerate(grads["v_biases"])]


def _assert_equal(out, grads, ref_out, ref_grads):
    assert torch.equal(out, ref_out.float()), f"forward differs in {(out != ref_out.float()).sum().item()} of {out.numel()} elements"
    for (name, got), (_, ref) in zip(_tensors(grads), _tensors(ref_grads)):
        assert got.shape == ref.shape, name
        wrong = got != ref.float()
        assert not bool(wrong.any()), f"{name}: {int(wrong.sum())} of {got.numel()} elements differ, first at {wrong.nonzero()[0].tolist()}"


EXACT_NETS = [(64, 32, 64, 3, 3), (64, 32, 64, 3, 4), (4, 5, 32, 2, 3), (4, 5, 32, 2, 4)]


@pytest.mark.parametrize("net", EXACT_NETS + [(32, 8, 32, 4, 4)], ids=lambda n: "F%d_E%d_H%d_L%d_out%d" % n)
def test_integer_cases_stay_exact_at_the_largest_row_count(net):
    """CPU: the bound the oracle asserts holds at the largest M, for every network of the exact tests."""
    assert 0 < _integer_case(_row_counts()[-1], *net)[4] < AO.EXACT_LIMIT


@gpu
@pytest.mark.parametrize("net", EXACT_NETS, ids=lambda n: "F%d_E%d_H%d_L%d_out%d" % n)
@pytest.mark.parametrize("which", range(8))
def test_exact_integers(net, which):
    N = _row_counts()[which]
    inputs, mask, ref_out, ref_grads, _ = _integer_case(N, *net)
    out, grads = _run(inputs, output_activation="none")
    _assert_equal(out, grads, ref_out, ref_grads)


@gpu
@pytest.mark.parametrize("which", [4, 6])
def test_exact_integers_four_layers(which):
    N = _row_counts()[which]
    inputs, mask, ref_out, ref_grads, _ = _integer_case(N, 32, 8, 32, 4, 4)
    out, grads = _run(inputs, output_activation="none")
    _assert_equal(out, grads, ref_out, ref_grads)


@gpu
@pytest.mark.parametrize("kind", ["none", "all", "nothing", "alternating", "last_of_block"])
def test_masks_exact_and_every_row_written(kind):
    """Integer data; the result buffers are NaN before the calls, so a masked row that the kernel did not write shows."""
    from gspl_amd.ops import appearance as A
    T, B, G = _constants()
    N, F, E, H, L, n_out = 2 * B + 5, 64, 32, 64, 3, 4
    inputs, mask, ref_out, ref_grads, _ = _integer_case(N, F, E, H, L, n_out, kind)
    features, weights, biases, embedding, v_out = [[u.to(DEV) for u in t] if isinstance(t, list) else t.to(DEV) for t in inputs]
    mask8 = None if mask is None else mask.to(DEV).view(torch.uint8)
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    out = A.appearance_mlp_forward(features, weights, biases, embedding, mask8, output_activation="none", out=nan(N, n_out))
    n_params = sum(w.numel() + b.numel() for w, b in zip(weights, biases)) + E
    v_features, v_params = A.appearance_mlp_backward(features, weights, biases, embedding, v_out, mask8, output_activation="none",
                                                     v_features=nan(N, F), v_params=nan(n_params))
    torch.cuda.synchronize()
    v_w, v_b, v_e = A.split_params(v_params.cpu(), weights, biases, E)
    grads = dict(v_features=v_features.cpu(), v_weights=v_w, v_biases=v_b, v_embedding=v_e)
    _assert_equal(out.cpu(), grads, ref_out, ref_grads)
    if kind == "nothing":
        assert not bool(out.any()) and not bool(v_features.any()) and not bool(v_params.any())


# ---- random parity ------------------------------------------------------------------------------------------------------------------------
def _random_case(N, F, E, H, L, n_out, n_freq, seed, zero_row=False):
    g = torch.Generator().manual_seed(seed)
    rand = lambda *shape: torch.randn(shape, generator=g)
    P = 3 * (2 * n_freq + 1) if n_freq else 0
    features = rand(N, F) * 0.5
    features += 0.25 * torch.sign(features)              # every row well away from zero norm
    if zero_row:
        features[N // 3] = 0
    weights, biases, fan_in = [], [], F + E + P
    for layer in range(L):
        rows = n_out if layer == L - 1 else H
        weights.append((torch.rand((rows, fan_in), generator=g) * 2 - 1) / fan_in ** 0.5)
        biases.append((torch.rand((rows,), generator=g) * 2 - 1) / fan_in ** 0.5)
        fan_in = H
    means, camera = rand(N, 3) * 2, torch.tensor([0.3, -0.2, 4.0])
    mask = torch.rand((N,), generator=g) < 0.7
    mask[N // 3] = True                                  # (the zero row is a visible one)
    return (features, weights, biases, rand(E), rand(N, n_out)), mask, means, camera


PARITY = {
    "default_E32": dict(N=4096, F=64, E=32, H=64, L=3, n_out=3, n_freq=0, normalize=False),
    "default_E128": dict(N=1500, F=64, E=128, H=64, L=3, n_out=3, n_freq=0, normalize=False),
    "view_dependent": dict(N=1100, F=64, E=32, H=64, L=3, n_out=3, n_freq=4, normalize=False),
    "view_dependent_normalize_out4": dict(N=1100, F=64, E=32, H=64, L=3, n_out=4, n_freq=4, normalize=True),
    "normalize": dict(N=777, F=64, E=32, H=64, L=3, n_out=4, n_freq=0, normalize=True),
    "F128": dict(N=600, F=128, E=32, H=64, L=3, n_out=3, n_freq=0, normalize=False),
    "F128_view_dependent_H32_L4": dict(N=600, F=128, E=16, H=32, L=4, n_out=4, n_freq=4, normalize=True),
}


@gpu
@pytest.mark.parametrize("name", list(PARITY))
def test_random_parity(name):
    case = dict(PARITY[name])
    normalize, n_freq = case.pop("normalize"), case["n_freq"]
    inputs, mask, means, camera = _random_case(seed=len(name), zero_row=normalize, **case)
    options = dict(n_view_frequencies=n_freq, normalize=normalize, output_activation="sigmoid")
    ref_out, cache = AO.forward(*inputs[:4], mask=mask, means=means, camera_center=camera, **options)
    ref_grads = AO.backward(cache, inputs[4])
    out, grads = _run(inputs, mask, means if n_freq else None, camera if n_freq else None, **options)
    assert bool(torch.isfinite(out).all())
    forward_error = float((out.double() - ref_out).abs().max())
    print(f"{name}: forward max |got - ref| = {forward_error:.3e}")
    worst = {}
    for (tensor, got), (_, ref) in zip(_tensors(grads), _tensors(ref_grads)):
        assert bool(torch.isfinite(got).all()), tensor
        bound = 1e-4 * (ref.abs() + ref.pow(2).mean().sqrt())
        worst[tensor] = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max()) if ref.numel() else 0.0
        print(f"{name}: {tensor} max error / bound = {worst[tensor]:.3e}")
    assert forward_error <= 1e-5
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- determinism, bounds, autograd ----------------------------------------------------------------------------------------------------------
@gpu
def test_backward_is_deterministic():
    T, B, G = _constants()
    case = dict(PARITY["view_dependent_normalize_out4"], N=3 * G * B // 2 + 11)
    normalize, n_freq = case.pop("normalize"), case["n_freq"]
    inputs, mask, means, camera = _random_case(seed=5, **case)
    options = dict(n_view_frequencies=n_freq, normalize=normalize)
    first = _run(inputs, mask, means, camera, **options)
    second = _run(inputs, mask, means, camera, **options)
    assert torch.equal(first[0], second[0])
    for (name, a), (_, b) in zip(_tensors(first[1]), _tensors(second[1])):
        assert torch.equal(a, b), name


@gpu
def test_guard_bands_stay_intact():
    """out, v_features and v_params sit between poisoned bands inside one plain tensor; forward and backward leave the bands alone."""
    from gspl_amd.ops import appearance as A
    N, F, E, H, L, n_out, band = 333, 64, 32, 64, 3, 3, 1024
    inputs, mask, means, camera = _random_case(N, F, E, H, L, n_out, 4, seed=9)
    features, weights, biases, embedding, v_out = [[u.to(DEV) for u in t] if isinstance(t, list) else t.to(DEV) for t in inputs]
    n_params = sum(w.numel() + b.numel() for w, b in zip(weights, biases)) + E
    sizes = [N * n_out, N * F, n_params]
    starts, at = [], band
    for size in sizes:
        starts.append(at)
        at += size + (-size) % 4 + band
    arena = torch.empty((at,), device=DEV)
    poison = torch.tensor(0x7FC0DEAD, dtype=torch.int32, device=DEV)
    arena.view(torch.int32).fill_(poison)
    out, v_features, v_params = [arena[s:s + n] for s, n in zip(starts, sizes)]
    mask8 = mask.to(DEV).view(torch.uint8)
    A.appearance_mlp_forward(features, weights, biases, embedding, mask8, means.to(DEV), camera.to(DEV), 4, out=out.view(N, n_out))
    A.appearance_mlp_backward(features, weights, biases, embedding, v_out, mask8, means.to(DEV), camera.to(DEV), 4,
                              v_features=v_features.view(N, F), v_params=v_params)
    torch.cuda.synchronize()
    words, lo = arena.view(torch.int32), 0
    for start, size in zip(starts, sizes):
        assert bool((words[lo:start] == poison).all()), f"the band [{lo}, {start}) was written"
        lo = start + size
    assert bool((words[lo + (-sizes[-1]) % 4:] == poison).all())
    assert all(bool(torch.isfinite(t).all()) for t in (out, v_features, v_params)) and bool(v_params.any())


@gpu
def test_non_contiguous_inputs_are_copied():
    from gspl_amd import ops
    inputs, mask, _, _ = _random_case(300, 64, 32, 64, 3, 3, 0, seed=2)
    features, weights, biases, embedding, v_out = [[u.to(DEV) for u in t] if isinstance(t, list) else t.to(DEV) for t in inputs]
    wide = torch.zeros((300, 128), device=DEV)
    wide[:, ::2] = features
    w0_t = weights[0].t().contiguous().t()
    assert not wide[:, ::2].is_contiguous() and not w0_t.is_contiguous()
    want = ops.appearance_mlp(features, weights, biases, embedding)
    got = ops.appearance_mlp(wide[:, ::2], [w0_t] + weights[1:], biases, embedding)
    assert torch.equal(want, got)


@gpu
def test_needs_input_grad_and_frozen_weights(monkeypatch):
    from gspl_amd import ops
    from gspl_amd.ops import appearance as A
    inputs, mask, _, _ = _random_case(300, 64, 32, 64, 3, 3, 0, seed=3)
    features, weights, biases, embedding, v_out = [[u.to(DEV) for u in t] if isinstance(t, list) else t.to(DEV) for t in inputs]
    calls = []
    real = A.L.call
    monkeypatch.setattr(A.L, "call", lambda name, *args: (calls.append((name, args)), real(name, *args))[1])
    names = A.L._FUNCTIONS["gspl_appearance_mlp_bwd"][2]

    # frozen network and embedding: only the features get a gradient, and the launch is told to skip the weight gradients
    f = features.clone().requires_grad_(True)
    ops.appearance_mlp(f, weights, biases, embedding).backward(v_out)
    bwd = [args for name, args in calls if name == "gspl_appearance_mlp_bwd"]
    assert len(bwd) == 1 and f.grad is not None
    assert bwd[0][names.index("v_params")] is None and bwd[0][names.index("workspace")] is None
    assert bwd[0][names.index("v_features")] is not None

    # features need none: no v_features buffer; one frozen layer gets no gradient, the others do
    calls.clear()
    ws = [w.clone().requires_grad_(i != 1) for i, w in enumerate(weights)]
    bs = [b.clone().requires_grad_(True) for b in biases]
    e = embedding.clone().requires_grad_(True)
    ops.appearance_mlp(features, ws, bs, e).backward(v_out)
    bwd = [args for name, args in calls if name == "gspl_appearance_mlp_bwd"]
    assert len(bwd) == 1 and bwd[0][names.index("v_features")] is None and bwd[0][names.index("v_params")] is not None
    assert ws[0].grad is not None and ws[1].grad is None and ws[2].grad is not None and e.grad is not None
    assert all(b.grad is not None for b in bs)

    # nothing needs a gradient: no backward launch at all
    calls.clear()
    out = ops.appearance_mlp(features, weights, biases, embedding)
    assert not out.requires_grad and [name for name, _ in calls] == ["gspl_appearance_mlp_fwd"]


@gpu
def test_cpu_tensors_and_unbuilt_options_are_refused_before_any_launch(monkeypatch):
    from gspl_amd import ops
    from gspl_amd.ops import appearance as A
    monkeypatch.setattr(A.L, "call", lambda *a: pytest.fail("a refused call reached the library"))
    inputs, _, _, _ = _random_case(10, 64, 32, 64, 3, 3, 0, seed=4)
    features, weights, biases, embedding, _ = inputs
    with pytest.raises(RuntimeError, match="GPU"):
        ops.appearance_mlp(features, weights, biases, embedding)
    with pytest.raises(NotImplementedError, match="output_activation"):
        ops.appearance_mlp(features.to(DEV), [w.to(DEV) for w in weights], [b.to(DEV) for b in biases], embedding.to(DEV), output_activation="relu")

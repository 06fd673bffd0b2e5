"""`ops.sh_view_opacities` (include/gspl_hip.h section 25, csrc/glossy.hip, ops/glossy.py) against the fp64 oracle tests/glossy_oracle.py,
which tests/test_glossy.py pins to the reference's own run.  Nothing here reads the reference tree.

Tolerances.  eps32 = 2^-23 (one ulp of 1.0; a rounded operation errs by at most half of it, so every count below has a factor 2 of room
for second-order terms).  The inputs are float32 values, which the oracle widens exactly.  With B_k the oracle's majorant of basis_k
(every monomial and constant by magnitude: the polynomials cancel, so their error is relative to B_k, not to |basis_k|) and L_k the
polynomial's degree:

  direction   a component of d passes 7 rounded operations (D_ROUNDINGS): the subtraction (1); the sum of squares carries 2 from its
              inputs and 3 of its own, halved by the square root (2.5) + the root (1) + the reciprocal (1) = 4.5; the product (1): 6.5.
  basis       |basis_k - ref| <= eps32 (7 L_k + 8) B_k: L_k factors of d, and at most 8 roundings along the longest product path of a
              polynomial, the float32 constant's own included (BASIS_ROUNDINGS; k = 24: 5 per product, the difference, the constant, its
              representation).  The direction's conditioning is this term.
  value       the chain is fl(C0) dc (2), one fmaf per further coefficient (K - 1) and the + 0.5 (1): c = K + 2, at most 27, and
                  |value - ref| <= eps32 [(K + 2) (|C0 dc| + sum_k |basis_k rest_k| + 0.5) + sum_k (7 L_k + 8) B_k |rest_k|]
              (the clamp is a contraction).
  gradient    v_dc = fl(C0) g: 2 eps32 |C0 g|;  v_rest_k = basis_k g: eps32 ((7 L_k + 8) B_k + |basis_k|) |g|, exact zeros above the
              active degree, where g = 0 and in clamped rows.
  near rows   a row whose oracle value before the clamp lies within the value bound of 0 or of 1 may take either branch in the
              gradient (its gradient row then equals the passing or the zero one within the bound).  They are counted and printed, and
              are at most 1e-3 of a case's rows.
The GPU tests never widen these."""
import functools
import os

import numpy as np
import pytest
import torch

import glossy_oracle as GO
from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)

DEV = "cuda:0"
EPS = GO.EPS32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_glossy.npz")
D_ROUNDINGS, BASIS_ROUNDINGS = 7, 8
NEAR_CAP = 1e-3
BLOCK = 256                                            # rows per workgroup (csrc/glossy.hip)
SIZES = [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 1000]
WIDTHS = [(degree, Kr) for Kr in (0, 3, 8, 15, 24) for degree in range(5) if (degree + 1) ** 2 - 1 <= Kr]
CAMERA = np.array([0.1, -0.2, 0.3], dtype=np.float32)


def _basis_slack(degree, o):
    """[N, K]: (7 L_k + 8) B_k"""
    K = (degree + 1) ** 2
    return (D_ROUNDINGS * GO.ORDER[:K] + BASIS_ROUNDINGS) * o["major"]


def value_bound(degree, o, rest):
    K = (degree + 1) ** 2
    rest = np.abs(np.asarray(rest, dtype=np.float64).reshape(o["raw"].shape[0], -1)[:, :K - 1])
    return EPS * ((K + 2) * o["mag"] + (_basis_slack(degree, o)[:, 1:] * rest).sum(axis=1))


def gradient_bounds(degree, o, g, Kr):
    """(bound of v_dc [N], bound of v_rest [N, Kr]) for the incoming gradient g (zero in the columns above the active degree)."""
    K = (degree + 1) ** 2
    g = np.abs(np.asarray(g, dtype=np.float64))
    rest = np.zeros((g.shape[0], Kr))
    rest[:, :K - 1] = EPS * (_basis_slack(degree, o) + np.abs(o["basis"]))[:, 1:] * g[:, None]
    return EPS * 2 * GO.C0 * g, rest


def draw(N, Kr, seed):
    """The law of the golden file: means uniform in [-1, 1]^3, dc 1.5 randn, rest 0.5 randn, row 7 AT the camera with dc = 0; the
    incoming gradient is randn with three rows in ten exactly zero (the invisible Gaussians)."""
    rng = np.random.default_rng(seed)
    means = rng.uniform(-1, 1, (N, 3)).astype(np.float32)
    dc = (1.5 * rng.standard_normal(N)).astype(np.float32)
    rest = (0.5 * rng.standard_normal((N, Kr))).astype(np.float32)
    w = (rng.standard_normal(N) * (rng.random(N) > 0.3)).astype(np.float32)
    if N > 7:
        means[7], dc[7], w[7] = CAMERA, 0.0, 1.0
    return means, dc, rest, w


@functools.lru_cache(maxsize=None)
def _case(degree, N, Kr):
    means, dc, rest, w = draw(N, Kr, 1000 * degree + 31 * Kr + N)
    return (means, dc, rest, w), GO.opacity(degree, means, CAMERA, dc, rest, w)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _run(degree, means, dc, rest, w):
    from gspl_amd import ops
    m, c, d, r, v = _dev(means, CAMERA, dc, rest, w)
    value = ops.sh_view_opacities_forward(degree, m, c, d, r)
    v_dc, v_rest = ops.sh_view_opacities_backward(degree, m, c, d, r, v)
    return value.cpu().numpy(), v_dc.cpu().numpy(), v_rest.cpu().numpy()


def _within(got, ref, bound, what):
    diff = np.abs(np.asarray(got, dtype=np.float64) - ref)
    ratio = (diff / np.maximum(bound, 1e-300)).max(initial=0.0)
    print(f"{what}: worst |diff| {diff.max(initial=0.0):.3e}, worst |diff| / bound = {ratio:.3f}")
    assert (diff <= bound).all(), f"{what}: |diff| / bound = {ratio:.3f}"
    return ratio


def check(degree, inputs, o, got, what):
    """Value, v_dc and v_rest against the oracle `o` under the counted bounds; returns the worst ratio to a bound."""
    means, dc, rest, w = inputs
    value, v_dc, v_rest = got
    N, Kr, K = dc.shape[0], rest.shape[1], (degree + 1) ** 2
    vb = value_bound(degree, o, rest)
    worst = _within(value, o["value"], vb, f"{what} value")
    near = (np.abs(o["raw"]) <= vb) | (np.abs(o["raw"] - 1.0) <= vb)
    print(f"{what}: {int(near.sum())} of {N} rows within the bound of a threshold")
    assert near.mean() <= NEAR_CAP
    firm = ~near
    db, rb = gradient_bounds(degree, o, w * ((o["raw"] >= 0) & (o["raw"] <= 1)), Kr)
    worst = max(worst, _within(v_dc[firm], o["v_dc"][firm], db[firm], f"{what} v_dc"), _within(v_rest[firm], o["v_rest"][firm], rb[firm], f"{what} v_rest"))
    for n in np.nonzero(near)[0]:              # either branch, whole
        passing = GO.opacity(degree, means[n:n + 1], CAMERA, dc[n:n + 1] * 0, rest[n:n + 1] * 0, w[n:n + 1])      # raw = 0.5: passes
        pd, pr = gradient_bounds(degree, passing, w[n:n + 1], Kr)
        zero = not v_dc[n] and not v_rest[n].any()
        assert zero or (abs(v_dc[n] - passing["v_dc"][0]) <= pd[0] and (np.abs(v_rest[n] - passing["v_rest"][0]) <= pr[0]).all()), f"{what}: row {n}"
    # exact zeros: above the active degree, where no gradient came in, where the clamp cut
    assert not v_rest[:, K - 1:].any()
    dead = firm & ((w == 0) | (o["raw"] < 0) | (o["raw"] > 1))
    assert not v_dc[dead].any() and not v_rest[dead].any()
    assert np.isfinite(value).all() and np.isfinite(v_dc).all() and np.isfinite(v_rest).all()
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("degree", range(5))
def test_wave_and_block_edges(degree, N):
    Kr = (degree + 1) ** 2 - 1
    inputs, o = _case(degree, N, Kr)
    check(degree, inputs, o, _run(degree, *inputs), f"degree {degree}, N {N}")


@pytest.mark.gpu
@pytest.mark.parametrize("degree,Kr", WIDTHS)
def test_row_widths(degree, Kr):
    """Kr 0 (the NULL pointer), 3, 8, 15 and 24 with every degree they hold, N = 257: rows wider than the active degree are staged by
    their first columns only."""
    inputs, o = _case(degree, BLOCK + 1, Kr)
    check(degree, inputs, o, _run(degree, *inputs), f"degree {degree}, Kr {Kr}")


@pytest.mark.gpu
@pytest.mark.parametrize("degree", range(5))
def test_the_golden_inputs(degree):
    """The reference's own rows: the kernel against the stored float64 run, through the oracle's bounds."""
    with np.load(GOLDEN) as z:
        means, dc, rest, w = (z[k].astype(np.float32) for k in ("means", "dc", "rest", "w"))
        stored = z[f"value{degree}"]
    dc, rest = dc.reshape(-1), rest[..., 0]
    o = GO.opacity(degree, means, CAMERA, dc, rest, w)
    got = _run(degree, means, dc, rest, w)
    check(degree, (means, dc, rest, w), o, got, f"golden, degree {degree}")
    _within(got[0], stored, value_bound(degree, o, rest), "against the stored run")


@pytest.mark.gpu
def test_columns_above_the_active_degree_are_not_read():
    """Kr = 15 at degree 1, the extra columns holding NaN: same bits as with zeros there, and zero gradients in them."""
    (means, dc, rest, w), o = _case(1, BLOCK + 1, 15)
    poisoned = rest.copy()
    poisoned[:, 3:] = np.nan
    clean, dirty = _run(1, means, dc, rest, w), _run(1, means, dc, poisoned, w)
    assert all(np.array_equal(a, b) for a, b in zip(clean, dirty))
    assert not dirty[2][:, 3:].any()
    check(1, (means, dc, rest, w), o, dirty, "poisoned columns")


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [0, 1, 4])
def test_the_zero_direction_row(degree):
    """Row 7 sits AT the camera: d = 0, no NaN; at degree 4 the value is 0.5 + 3 C4[4] rest[7, 19], as the reference has it."""
    Kr = (degree + 1) ** 2 - 1
    (means, dc, rest, w), o = _case(degree, 65, Kr)
    value, v_dc, v_rest = _run(degree, means, dc, rest, w)
    assert np.array_equal(means[7], CAMERA) and not o["d"][7].any()
    expected = 0.5 + (3 * GO.C4[4] * float(rest[7, 19]) if degree == 4 else 0.0)
    assert abs(o["raw"][7] - expected) <= 1e-15 and 0 < expected < 1
    assert np.isfinite(value[7]) and abs(value[7] - expected) <= value_bound(degree, o, rest)[7]
    assert abs(v_dc[7] - GO.C0) <= 2 * EPS * GO.C0                      # w[7] = 1
    if degree == 4:
        want = np.zeros(24)
        want[19] = 3 * GO.C4[4]
        assert np.abs(v_rest[7] - want).max() <= EPS * (BASIS_ROUNDINGS + 1) * 3 * GO.C4[4] and v_rest[7, 19] != 0


@pytest.mark.gpu
def test_zero_and_sparse_incoming_gradients():
    """All zero in -> all zero out; a sparse gradient gives, on the rows that have one, the bits of the dense computation, and zeros
    elsewhere (those rows' coefficients are not read: NaN there changes nothing)."""
    (means, dc, rest, w), _ = _case(3, 1000, 15)
    _, v_dc, v_rest = _run(3, means, dc, rest, np.zeros_like(w))
    assert not v_dc.any() and not v_rest.any()
    dense = np.where(w == 0, np.float32(0.7), w)
    keep = np.zeros(1000, dtype=bool)
    keep[[3, 64, 255, 256, 300, 511, 999]] = True
    keep[600:700] = True
    sparse = np.where(keep, dense, np.float32(0))
    _, d_dc, d_rest = _run(3, means, dc, rest, dense)
    poisoned = rest.copy()
    poisoned[~keep] = np.nan
    _, s_dc, s_rest = _run(3, means, dc, poisoned, sparse)
    assert np.array_equal(s_dc[keep], d_dc[keep]) and np.array_equal(s_rest[keep], d_rest[keep]) and d_rest[keep].any()
    assert not s_dc[~keep].any() and not s_rest[~keep].any()


@pytest.mark.gpu
def test_two_runs_give_the_same_bits():
    (means, dc, rest, w), _ = _case(4, 1000, 24)
    a, b = _run(4, means, dc, rest, w), _run(4, means, dc, rest, w)
    assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def _between_bands(fill_byte, degree, N, Kr, misalign=0):
    """Forward and backward into caller buffers between poisoned bands (the arena of tests/test_spotless_plugin_gpu.py); misalign: the
    coefficient rows and their gradients start that many floats off a 16-byte boundary (the kernels' 4-byte path)."""
    from gspl_amd import ops
    from test_spotless_plugin_gpu import _arena
    (means, dc, rest, w), o = _case(degree, N, Kr)
    sizes = [N, N, N * Kr + misalign, N * Kr + misalign]                 # value, v_dc, v_rest, and the coefficients themselves
    arena, starts, poison = _arena(sizes)
    slots = [arena[s:s + n] for s, n in zip(starts, sizes)]
    for slot in slots:
        slot.view(torch.uint8).fill_(fill_byte)
    value, v_dc = slots[0], slots[1]
    v_rest, r = slots[2][misalign:].view(N, Kr), slots[3][misalign:].view(N, Kr)
    m, c, d, v = _dev(means, CAMERA, dc, w)
    r.copy_(torch.from_numpy(rest))
    assert r.data_ptr() % 16 == 4 * misalign and v_rest.data_ptr() % 16 == 4 * misalign
    ops.sh_view_opacities_forward(degree, m, c, d, r, out=value)
    ops.sh_view_opacities_backward(degree, m, c, d, r, v, v_dc=v_dc, v_rest=v_rest)
    torch.cuda.synchronize()
    words = arena.view(torch.int32)
    edges = [0] + [e for s, n in zip(starts, sizes) for e in (s, s + n)] + [arena.numel()]
    for lo, hi in zip(edges[0::2], edges[1::2]):
        assert bool((words[lo:hi] == poison).all()), f"the band [{lo}, {hi}) was written"
    for slot in slots[2:]:                                               # the floats in front of a misaligned array keep the fill
        assert bool((slot[:misalign].view(torch.uint8) == fill_byte).all())
    got = [value.cpu().numpy(), v_dc.cpu().numpy(), v_rest.cpu().numpy()]
    check(degree, (means, dc, rest, w), o, got, f"between bands, degree {degree}, offset {misalign}")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [0, 1])
def test_guard_bands_stay_intact_and_prefill_does_not_matter(misalign):
    """Kr = 15, N = 257: the odd row stride is where an overrun would land."""
    a, b = _between_bands(0xFF, 3, BLOCK + 1, 15, misalign), _between_bands(0x00, 3, BLOCK + 1, 15, misalign)
    assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))
    plain = _run(3, *_case(3, BLOCK + 1, 15)[0])
    assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, plain))      # 16-byte and 4-byte paths agree


@pytest.mark.gpu
def test_autograd_shapes_layouts_and_targets():
    """`sh_view_opacities`: the model's shapes in, gradients in those shapes out with the bits of the launches alone; means and camera
    get none; a non-contiguous input is copied and changes nothing; N = 0 is an empty result."""
    from gspl_amd import ops
    (means, dc, rest, w), _ = _case(3, 1000, 15)
    _, want_dc, want_rest = _run(3, means, dc, rest, w)
    m, c, d, r, v = _dev(means, CAMERA, dc, rest, w)
    for dshape, rshape in (((1000, 1, 1), (1000, 15, 1)), ((1000, 1), (1000, 15)), ((1000,), (1000, 15))):
        mm, cc = m.clone().requires_grad_(True), c.clone().requires_grad_(True)
        dd, rr = d.reshape(dshape).clone().requires_grad_(True), r.reshape(rshape).clone().requires_grad_(True)
        out = ops.sh_view_opacities(3, mm, cc, dd, rr)
        assert tuple(out.shape) == (1000,)
        (out * v).sum().backward()
        assert tuple(dd.grad.shape) == dshape and tuple(rr.grad.shape) == rshape and mm.grad is None and cc.grad is None
        assert np.array_equal(dd.grad.reshape(-1).cpu().numpy(), want_dc) and np.array_equal(rr.grad.reshape(1000, 15).cpu().numpy(), want_rest)
    wide = torch.zeros(1000, 20, device=DEV)
    wide[:, :15] = r
    strided = ops.sh_view_opacities_forward(3, m, c, torch.stack([d, d], dim=1)[:, 0], wide[:, :15])
    assert torch.equal(strided, ops.sh_view_opacities_forward(3, m, c, d, r))
    empty = ops.sh_view_opacities(2, m[:0], c, d[:0], r[:0])
    assert tuple(empty.shape) == (0,)


@pytest.mark.gpu
def test_a_deferred_update_of_the_coefficients_is_awaited():
    """`opacity_rest` under `FusedAdam(deferred=...)`: the op launched right after a step gives what it gives once the device has been
    synchronised (it waits for the update's event, as `sh_view_colors` does)."""
    from gspl_amd import ops
    from gspl_amd.optimizers import FusedAdam
    n = 400000
    g = torch.Generator().manual_seed(5)
    means = (torch.rand(n, 3, generator=g) * 2 - 1).to(DEV)
    camera = torch.from_numpy(CAMERA).to(DEV)
    dc = torch.randn(n, 1, 1, generator=g).to(DEV).requires_grad_(True)
    rest = (0.5 * torch.randn(n, 15, 1, generator=g)).to(DEV).requires_grad_(True)
    opt = FusedAdam([{"params": [dc], "lr": 1e-2, "name": "opacities"}, {"params": [rest], "lr": 1e-2, "name": "opacity_rest"}], eps=1e-15,
                    deferred=("opacity_rest",))

    def read():
        with torch.no_grad():
            return ops.sh_view_opacities(3, means, camera, dc, rest)

    before = read()
    try:
        for it in range(3):
            dc.grad, rest.grad = torch.randn(dc.shape, generator=g).to(DEV), torch.randn(rest.shape, generator=g).to(DEV)
            torch.cuda.synchronize()
            opt.step()
            first = read()
            torch.cuda.synchronize()
            assert rest.data_ptr() in ops.PENDING_UPDATES
            settled = read()
            assert torch.equal(first, settled), f"step {it}: the op read opacity_rest before its update had finished"
            assert not torch.equal(settled, before)
            before = settled
    finally:
        opt.join()

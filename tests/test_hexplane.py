"""The HexPlane field (include/gspl_hip.h section 22, csrc/hexplane.hip, ops/hexplane.py) against the oracle tests/hexplane_oracle.py,
which tests/test_gs4d_shims.py pins to the reference's own double-precision run.

Tolerances, with u = 2^-24 (half an ulp of 1 in float32) and the oracle's own sums of magnitudes; each constant is the count of rounded
float32 operations a term passes through in the kernel, plus one for the second-order terms:
  forward   |out - ref| <= 48 u prod_p A_p, A_p = sum over the corners of |w v|.
            A weight is (1 - f_a)(1 - f_b): 3 roundings; a plane is one product and three fmas: its first term passes 4 more, 7 per plane,
            42 for six planes; 5 multiplications join them: 47.
  v_table   exactly 0 wherever no point with a non-zero gradient reaches the texel (this pins index, clamp and plane order); elsewhere
            |v - ref| <= (count + 46) u sum |w g prod_{q != p} I_q|: the five other planes (35) joined by 5 multiplications, times g (1),
            times the weight (3 + 1): 45 per contribution, and `count` additions in an order the atomics choose.
            The sum is taken over |I_q|, not A_q: it bounds the rounding of I_q only where the four corner values of a cell share a sign,
            so every plane of the tables here has ONE sign per channel (both signs occur; magnitudes in [0.1, 1], where the reference's
            initialisation puts them).
  v_x       |v - ref| <= 72 u sum over levels, channels, planes holding the axis and corners of |pixels-per-unit g w_other v prod I_q|:
            a corner difference, (1 - f), their product and an fma (4); the other planes and g (41); 12 fmas into the level's sum; the
            pixels-per-unit factor (1); up to 8 levels (8); a butterfly of up to 4 additions over the lanes of a point: 70.
The GPU tests never widen these.  The oracle computes the pixel coordinates in float32 in the documented order, so kernel and oracle take
the same cell for every input and no input is excluded."""
import functools

import numpy as np
import pytest
import torch

import hexplane_oracle as HO
from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)

DEV = "cuda:0"
U = HO.U
K_FWD, C_TABLE, K_X = 48, 46, 72
RES = [5, 6, 7, 3]          # all different: an axis swap cannot hide
MULTIRES = [1, 2, 4, 8]
AABB2 = np.array([[2.0] * 3, [-2.0] * 3], dtype=np.float32)          # a power of two: exact coordinates


def _layouts(F, L, res=RES):
    from gspl_amd import ops
    return ops.hexplane_layout(res, MULTIRES[:L], F), HO.layout(res, MULTIRES[:L], F)


def _table(olay, seed):
    """Magnitudes in [0.1, 1]; one sign per (plane, channel)."""
    rng = np.random.default_rng(seed)
    table = (rng.random((olay.total, olay.F), dtype=np.float32) * 0.9 + 0.1).astype(np.float32)
    for row in olay.planes:
        for a, b, Ra, Rb, first in row:
            table[first:first + Ra * Rb] *= rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=olay.F)
    return table


def _t_dev(t):
    return torch.from_numpy(np.ascontiguousarray(t)).to(DEV) if isinstance(t, np.ndarray) else float(t)


def _gpu(x, t, table, lay, aabb, v_out=None, want_x=False):
    from gspl_amd import ops
    xd, td, box = torch.from_numpy(x).to(DEV), torch.from_numpy(table).to(DEV), ops.hexplane_box(aabb)
    out = ops.hexplane_forward(xd, _t_dev(t), td, box, lay)
    if v_out is None:
        return out.cpu().numpy(), None, None
    v_table, v_x = ops.hexplane_backward(xd, _t_dev(t), td, box, lay, torch.from_numpy(v_out).to(DEV), torch.zeros_like(td), want_x)
    return out.cpu().numpy(), v_table.cpu().numpy(), None if v_x is None else v_x.cpu().numpy()


def _within(got, ref, bound, what):
    excess = np.abs(got.astype(np.float64) - ref) - bound
    worst = np.unravel_index(np.argmax(excess), excess.shape) if excess.size else None
    if excess.size:
        ratio = np.abs(got.astype(np.float64) - ref) / np.maximum(bound, 1e-300)
        print(f"{what}: worst |diff| / bound = {ratio[bound > 0].max() if (bound > 0).any() else 0.0:.3f}")
    assert excess.size == 0 or excess.max() <= 0, f"{what}: |diff| {abs(got[worst] - ref[worst]):.3e} > bound {bound[worst]:.3e} at {worst}"


def _check(x, t, table, lay, olay, aabb, v_out, want_x=True, ref=None):
    ref = ref or HO.encode(x, t, table, aabb, olay, v_out, want_x)
    out, v_table, v_x = _gpu(x, t, table, lay, aabb, v_out, want_x)
    _within(out, ref.out, K_FWD * U * ref.out_abs, "out")
    untouched = ref.v_table_count == 0
    assert not v_table[untouched].any(), f"{int((v_table[untouched] != 0).sum())} table entries no point reaches have a gradient"
    _within(v_table, ref.v_table, (ref.v_table_count + C_TABLE) * U * ref.v_table_abs, "v_table")
    if want_x:
        _within(v_x, ref.v_x, K_X * U * ref.v_x_abs, "v_x")
    return ref, (out, v_table, v_x)


def _exact_points(N, seed):
    """Multiples of 2^-6 in [-3, 3] with bounds 2: inside, outside, and exactly on the first and the last texel; t multiples of 2^-6 in
    [-1.5, 1.5] with t = 1 (the last texel) and |t| > 1.  With R - 1 < 2^8 every float32 step of the coordinate is exact."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-192, 193, size=(N, 3)) / 64.0).astype(np.float32)
    t = (rng.integers(-96, 97, size=N) / 64.0).astype(np.float32)
    if N >= 8:
        x[0], x[1], x[2], x[3] = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), (-2.0, 0.5, 2.0), (2.75, -2.0, -3.0)
        t[0], t[1], t[2], t[3] = 1.0, -1.0, 1.25, -1.5
    else:
        x[0], t[0] = (-2.0, 0.515625, 2.5), 1.0
    return x, t


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2, 4])
@pytest.mark.parametrize("F", [8, 16, 32, 64])
def test_exact_coordinates(F, L):
    """A lone point, a partial wave and several blocks; per-point times.  Every pixel coordinate is exact in float32, so the cells agree
    with the oracle's by construction and the discrete rules (index, clamp, the absent corner on the last texel, the plane order and
    [R_b, R_a]) are compared without any rounding in the coordinates."""
    lay, olay = _layouts(F, L)
    assert max(max(r) for r in olay.resolutions) - 1 < 2 ** 8
    table = _table(olay, 100 + F + L)
    for N in (1, 63, 1000):
        x, t = _exact_points(N, N)
        v_out = np.random.default_rng(N + 1).standard_normal((N, L * F)).astype(np.float32)
        ref, (out, _, _) = _check(x, t, table, lay, olay, AABB2, v_out)
        assert out.shape == (N, L * F) and ref.out_abs.min() > 0
        if N == 1000:
            assert (np.abs(x) > 2).any(axis=1).sum() > 100 and (np.abs(t) > 1).sum() > 100


@pytest.mark.gpu
@pytest.mark.parametrize("F", [8, 64])
def test_uniform_time_is_the_same_time_per_point(F):
    from gspl_amd import ops
    lay, olay = _layouts(F, 2)
    table = _table(olay, 3)
    x, _ = _exact_points(333, 5)
    v_out = np.random.default_rng(6).standard_normal((333, 2 * F)).astype(np.float32)
    for time in (0.640625, 1.0, -1.25):
        per_point = np.full(333, time, dtype=np.float32)
        ref, (out_p, v_table_p, v_x_p) = _check(x, per_point, table, lay, olay, AABB2, v_out)
        _, (out_u, v_table_u, v_x_u) = _check(x, time, table, lay, olay, AABB2, v_out, ref=ref)
        assert np.array_equal(out_u, out_p) and np.array_equal(v_x_u, v_x_p)
    with pytest.raises(ValueError, match="t must be"):
        ops.hexplane_forward(torch.zeros(4, 3, device=DEV), torch.zeros(3, device=DEV), torch.from_numpy(table).to(DEV), ops.hexplane_box(AABB2), lay)


@functools.lru_cache(maxsize=None)
def _random_case(F):
    """4096 random float32 points in and around a box that is no power of two (the reference's 1.6), random times, 30 % of the gradient
    rows zero.  No input is excluded."""
    lay, olay = _layouts(F, 2)
    aabb = np.array([[1.6] * 3, [-1.6] * 3], dtype=np.float32)
    rng = np.random.default_rng(0)
    x = ((rng.random((4096, 3), dtype=np.float32) * 2 - 1) * np.float32(2.1)).astype(np.float32)
    t = ((rng.random(4096, dtype=np.float32) * 2 - 1) * np.float32(1.25)).astype(np.float32)
    v_out = rng.standard_normal((4096, 2 * F)).astype(np.float32)
    zero = rng.random(4096) < 0.3
    v_out[zero] = 0.0
    table = _table(olay, 7)
    return lay, olay, aabb, x, t, table, v_out, zero, HO.encode(x, t, table, aabb, olay, v_out, True)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [8, 32])
def test_random_inputs(F):
    lay, olay, aabb, x, t, table, v_out, zero, ref = _random_case(F)
    assert (np.abs(x) > 1.6).any(axis=1).sum() > 1000 and (np.abs(x) < 1.6).all(axis=1).sum() > 1000
    _, (out, v_table, v_x) = _check(x, t, table, lay, olay, aabb, v_out, ref=ref)
    assert not v_x[zero].any() and v_x[~zero].any(axis=1).sum() > 2000          # (a point outside along all three axes has none)
    # the points whose gradient row is zero must not change v_table: the run on the other points alone gives the same, within the bound
    bound = (ref.v_table_count + C_TABLE) * U * ref.v_table_abs
    _, alone, _ = _gpu(np.ascontiguousarray(x[~zero]), np.ascontiguousarray(t[~zero]), table, lay, aabb, np.ascontiguousarray(v_out[~zero]))
    _within(alone, ref.v_table, bound, "v_table of the non-zero rows alone")
    assert not alone[ref.v_table_count == 0].any()


@pytest.mark.gpu
def test_contention_and_zero_rows():
    """256 points inside ONE cell of every plane of level 0 (each adds to the same four rows of each plane: the atomics must lose
    nothing), then a gradient that is zero everywhere: the caller's buffer keeps its bits."""
    from gspl_amd import ops
    lay, olay = _layouts(32, 2)
    rng = np.random.default_rng(11)
    x = (0.45 + 0.18 * rng.random((256, 3), dtype=np.float32)).astype(np.float32)
    t = (0.1 + 0.5 * rng.random(256, dtype=np.float32)).astype(np.float32)
    cells = [HO.pixels(HO.coordinates(x, t, AABB2)[0][:, d], olay.resolutions[0][d])[0] for d in range(4)]
    assert all(len(set(c.tolist())) == 1 for c in cells)
    v_out = rng.standard_normal((256, 64)).astype(np.float32)
    table = _table(olay, 12)
    ref, _ = _check(x, t, table, lay, olay, AABB2, v_out)
    first = olay.planes[1][0][4]
    assert sorted(set(ref.v_table_count[:first, 0].tolist())) == [0, 256]
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(table).to(DEV)
    buffer = torch.full_like(td, 1.5)
    ops.hexplane_backward(xd, torch.from_numpy(t).to(DEV), td, ops.hexplane_box(AABB2), lay, torch.zeros((256, 64), device=DEV), buffer)
    assert bool((buffer == 1.5).all())
    # v_table ACCUMULATES: a second backward into the same buffer gives the gradient of the points taken twice
    buffer.zero_()
    for _ in range(2):
        ops.hexplane_backward(xd, torch.from_numpy(t).to(DEV), td, ops.hexplane_box(AABB2), lay, torch.from_numpy(v_out).to(DEV), buffer)
    twice = HO.encode(np.concatenate([x, x]), np.concatenate([t, t]), table, AABB2, olay, np.concatenate([v_out, v_out]))
    _within(buffer.cpu().numpy(), twice.v_table, (twice.v_table_count + C_TABLE) * U * twice.v_table_abs, "v_table after two calls")


@pytest.mark.gpu
def test_autograd_reaches_the_reference_shaped_parameters():
    """`hexplane_pack` + `hexplane_encode` under torch.autograd: the gradient arrives in every [1, F, R_b, R_a] parameter, and in x only
    when x asks for it."""
    from gspl_amd import ops
    lay, olay = _layouts(16, 2)
    table = _table(olay, 22)
    rng = np.random.default_rng(21)
    x = ((rng.random((300, 3), dtype=np.float32) * 2 - 1) * np.float32(2.5)).astype(np.float32)
    v_out = rng.standard_normal((300, 32)).astype(np.float32)
    ref = HO.encode(x, 0.375, table, AABB2, olay, v_out, True)
    planes = [[torch.from_numpy(np.ascontiguousarray(table[first:first + Ra * Rb].reshape(Rb, Ra, 16).transpose(2, 0, 1)[None])).to(DEV).requires_grad_(True)
               for a, b, Ra, Rb, first in row] for row in olay.planes]
    wide = torch.zeros((300, 5), device=DEV)
    wide[:, 1:4] = torch.from_numpy(x).to(DEV)
    xs = wide[:, 1:4]                                    # not contiguous: copied
    packed = ops.hexplane_pack(planes, lay)
    assert np.array_equal(packed.detach().cpu().numpy(), table)
    out = ops.hexplane_encode(xs, 0.375, packed, torch.from_numpy(AABB2).to(DEV), lay)
    out.backward(torch.from_numpy(v_out).to(DEV))
    _within(out.detach().cpu().numpy(), ref.out, K_FWD * U * ref.out_abs, "out")
    assert wide.grad is None
    bound = (ref.v_table_count + C_TABLE) * U * ref.v_table_abs
    for row, grids in zip(olay.planes, planes):
        for (a, b, Ra, Rb, first), grid in zip(row, grids):
            got = grid.grad[0].permute(1, 2, 0).reshape(Ra * Rb, 16).cpu().numpy()
            _within(got, ref.v_table[first:first + Ra * Rb], bound[first:first + Ra * Rb], f"grad of plane ({a}, {b})")
    xg = torch.from_numpy(x).to(DEV).requires_grad_(True)
    ops.hexplane_encode(xg, 0.375, packed.detach(), AABB2, lay).backward(torch.from_numpy(v_out).to(DEV))
    _within(xg.grad.cpu().numpy(), ref.v_x, K_X * U * ref.v_x_abs, "x.grad")
    with pytest.raises(NotImplementedError, match="x must be float32"):
        ops.hexplane_encode(xg.detach().double(), 0.375, packed.detach(), AABB2, lay)
    with pytest.raises(NotImplementedError, match="table must be float32"):
        ops.hexplane_encode(xg.detach(), 0.375, packed.detach().double(), AABB2, lay)
    with pytest.raises(ValueError, match="x must be"):
        ops.hexplane_encode(xg.detach()[:, :2], 0.375, packed.detach(), AABB2, lay)
    with pytest.raises(ValueError, match="table must be"):
        ops.hexplane_encode(xg.detach(), 0.375, packed.detach()[:-1], AABB2, lay)

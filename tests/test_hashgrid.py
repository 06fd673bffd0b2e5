"""The multiresolution hash-grid / dense-grid encoding (include/gspl_hip.h section 20, csrc/hashgrid.hip, ops/hashgrid.py) against the
fp64 oracle tests/hashgrid_oracle.py.

Tolerances, with u = 2^-24 (half an ulp of 1 in float32) and the oracle's own sums of magnitudes:
  forward     |out - ref| <= 8 u sum |w t|: eight corner terms, each with a weight of up to three rounded factors, summed in float32
  v_table     exactly 0 where no (point, level) with a non-zero gradient reaches the entry (this pins the index, hash, modulo and wrap
              rules); elsewhere |v - ref| <= (count + 2) u sum |w g|: `count` additions in an order the atomics choose, plus the weight
  v_x         |v - ref| <= 8 u sum_l scale_l sum_corners |other weights| sum_f |t g|
The GPU tests never widen these; the shapes are the smallest that reach every path (dense and hashed levels, D = 2 and 3, every F,
a partial last block, more than one block, a wave whose points share one row)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import hashgrid_oracle as HO
from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
U = HO.U
SWAG_SCALE = math.exp((math.log(2048) - math.log(16)) / 11)


# ---- no GPU ------------------------------------------------------------------------------------------------------------------------------
def _both_tables(*args, **kw):
    from gspl_amd import ops
    lv, olv = ops.hashgrid_levels(*args, **kw), HO.levels(*args, **kw)
    assert lv.resolutions.tolist() == list(olv.resolutions) and lv.sizes.tolist() == list(olv.sizes)
    assert lv.offsets.tolist() == list(olv.offsets) + [olv.total] and lv.hashed.tolist() == list(olv.hashed) and lv.total == olv.total
    assert lv.scales.dtype == np.float32 and lv.scales.tolist() == [float(s) for s in olv.scales]
    assert lv.resolutions.dtype == np.uint32 and lv.offsets.dtype == np.uint32
    return lv


def test_level_table_of_swags_defaults():
    lv = _both_tables(3, 12, 4, 19, 16, SWAG_SCALE)
    assert lv.resolutions.tolist() == [16, 25, 39, 61, 94, 146, 226, 351, 546, 848, 1318, 2048]
    assert lv.sizes.tolist() == [4096, 15632, 59320, 226984] + [524288] * 8
    assert lv.hashed.tolist() == [False] * 4 + [True] * 8
    assert lv.total == 4500336 and lv.n_output_dims == 48 and lv.n_params == 4 * 4500336
    assert float(lv.scales[0]) == 15.0 and float(lv.scales[11]) == 2047.0


def test_level_table_of_the_small_grid():
    lv = _both_tables(3, 5, 2, 9, 4, 2.0)
    assert lv.resolutions.tolist() == [4, 8, 16, 32, 64] and lv.sizes.tolist() == [64, 512, 512, 512, 512]
    assert lv.hashed.tolist() == [False, False, True, True, True]          # level 1 is exactly full: dense
    assert lv.total == 2112 and lv.scales.tolist() == [3.0, 7.0, 15.0, 31.0, 63.0]
    dense = _both_tables(3, 5, 2, 9, 4, 2.0, dense=True)
    assert dense.sizes.tolist() == [64, 512, 4096, 32768, 262144] and not dense.hashed.any()
    flat = _both_tables(2, 3, 1, 4, 3, 1.5)
    assert flat.resolutions.tolist() == [3, 5, 7] and flat.sizes.tolist() == [16, 16, 16] and flat.hashed.tolist() == [False, True, True]


def test_level_table_refusals_name_the_parameter():
    from gspl_amd import ops
    for args, name in (((4, 5, 2, 9, 4, 2.0), "n_input_dims"), ((3, 0, 2, 9, 4, 2.0), "n_levels"), ((3, 33, 2, 9, 4, 2.0), "n_levels"),
                       ((3, 5, 3, 9, 4, 2.0), "n_features_per_level"), ((3, 5, 2, 40, 4, 2.0), "log2_hashmap_size"),
                       ((3, 5, 2, 9, 0, 2.0), "base_resolution"), ((3, 5, 2, 9, 4, 0.0), "per_level_scale")):
        with pytest.raises((ValueError, NotImplementedError), match=name):
            ops.hashgrid_levels(*args)
    with pytest.raises(ValueError, match="dense level"):
        ops.hashgrid_levels(3, 12, 2, 19, 16, 2.0, dense=True)


def test_header_declares_the_entry_points():
    from gspl_amd import _lib as L
    text = open(L.HEADER_PATH).read()
    for name in ("gspl_hashgrid_fwd", "gspl_hashgrid_bwd"):
        assert f"int {name}(" in text and name in L.exported_symbols()
    section = text[text.index(" 20. Multiresolution hash-grid"):]
    assert "20." in section and "PURELY ADDITIVE" in section and "UNPINNED" in section and L.ABI_VERSION == 39
    assert L._FUNCTIONS["gspl_hashgrid_fwd"][2] == ("N", "D", "F", "L", "scales", "resolutions", "offsets", "x", "table", "out", "stream")
    assert L._FUNCTIONS["gspl_hashgrid_bwd"][2][-5:] == ("table", "v_out", "v_table", "v_x", "stream")
    assert "hashgrid.hip" in open(os.path.join(ROOT, "gaussian-splatting-lightning_amd", "csrc", "Makefile")).read()


def test_cpu_tensors_and_bad_arguments_are_refused():
    from gspl_amd import ops
    lv = ops.hashgrid_levels(3, 5, 2, 9, 4, 2.0)
    table = ops.hashgrid_table(lv, seed=3)
    assert table.shape == (lv.n_params,) and table.dtype == torch.float32 and float(table.abs().max()) <= 1e-4
    assert torch.equal(table, ops.hashgrid_table(lv, seed=3)) and not torch.equal(table, ops.hashgrid_table(lv, seed=4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.hashgrid_encode(torch.zeros(4, 3), table, lv)
    with pytest.raises(TypeError, match="levels"):
        ops.hashgrid_encode(torch.zeros(4, 3), table, None)


def test_oracle_partition_of_unity_and_scatter():
    """The oracle's own sanity: a constant table encodes to the constant, the table gradient sums to the output gradient's sum, and
    v_x is the finite difference of the output (inside a cell the encoding is multilinear)."""
    olv = HO.levels(3, 5, 2, 9, 4, 2.0)
    rng = np.random.default_rng(1)
    x = rng.random((200, 3), dtype=np.float32)
    r = HO.encode(x, np.full((olv.total, 2), 0.25), olv)
    assert np.abs(r.out - 0.25).max() < 1e-14 and np.abs(r.out_abs - 0.25).max() < 1e-14
    table, v = rng.standard_normal((olv.total, 2)), rng.standard_normal((200, 10))
    # odd multiples of 2^-11: with the integer scales every pos is exact, no frac is 0, and a step of 2^-18 stays inside the cell
    x = ((2 * rng.integers(0, 1024, size=(200, 3)) + 1) / 2048.0).astype(np.float32)
    assert HO.min_frac_margin(x, olv) .min() >= 2.0 ** -11
    r = HO.encode(x, table, olv, v, want_x=True)
    assert abs(r.v_table.sum() - v.sum()) < 1e-9 and int(r.v_table_count.sum()) == 200 * 5 * 8 * 2
    step = np.float32(2.0 ** -18)
    for d in range(3):
        bump = np.zeros(3, dtype=np.float32)
        bump[d] = step
        fd = ((HO.encode(x + bump, table, olv).out - HO.encode(x - bump, table, olv).out) * v).sum(axis=1) / (2.0 * float(step))
        assert np.abs(fd - r.v_x[:, d]).max() <= 1e-8 * r.v_x_abs[:, d].max()
    assert HO.positions(np.array([[-0.25, 1.5, -1.0]], dtype=np.float32), np.float32(3.0))[0].tolist() == [[0xFFFFFFFF, 5, 0xFFFFFFFD]]


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def _grid(D, L, F, log2, base, scale, dense=False):
    from gspl_amd import ops
    return ops.hashgrid_levels(D, L, F, log2, base, scale, dense=dense), HO.levels(D, L, F, log2, base, scale, dense=dense)


def _tables(olv, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((olv.total, olv.F), dtype=np.float32) * 2 - 1)


def _gpu(x, table, lv, v_out=None, want_x=False):
    from gspl_amd import ops
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(table).to(DEV)
    out = ops.hashgrid_forward(xd, td, lv)
    if v_out is None:
        return out.cpu().numpy(), None, None
    v_table, v_x = ops.hashgrid_backward(xd, td, lv, torch.from_numpy(v_out).to(DEV), torch.zeros_like(td), want_x)
    return out.cpu().numpy(), v_table.cpu().numpy(), None if v_x is None else v_x.cpu().numpy()


def _within(got, ref, bound, what):
    excess = np.abs(got.astype(np.float64) - ref) - bound
    worst = np.unravel_index(np.argmax(excess), excess.shape) if excess.size else None
    assert excess.size == 0 or excess.max() <= 0, f"{what}: |diff| {abs(got[worst] - ref[worst]):.3e} > bound {bound[worst]:.3e} at {worst}"


def _check(x, table, lv, olv, v_out, want_x=False, ref=None):
    ref = ref or HO.encode(x, table, olv, v_out, want_x)
    out, v_table, v_x = _gpu(x, table, lv, v_out, want_x)
    _within(out, ref.out, 8 * U * ref.out_abs, "out")
    untouched = ref.v_table_count == 0
    assert not v_table[untouched].any(), f"{int((v_table[untouched] != 0).sum())} table entries no point reaches have a gradient"
    _within(v_table, ref.v_table, (ref.v_table_count + 2) * U * ref.v_table_abs, "v_table")
    if want_x:
        _within(v_x, ref.v_x, 8 * U * ref.v_x_abs, "v_x")
    return ref, (out, v_table, v_x)


def _lattice(D, seed=0):
    """x = k / 64 on {0 .. 64}^D: about 4 k points (all of them for D = 2) that include every face, plus 64 points outside [0, 1]."""
    rng = np.random.default_rng(seed)
    if D == 2:
        k = np.stack(np.meshgrid(np.arange(65), np.arange(65), indexing="ij"), axis=-1).reshape(-1, 2)
    else:
        k = rng.integers(0, 65, size=(3800, 3))
        faces = rng.integers(0, 65, size=(300, 3))
        faces[np.arange(300), rng.integers(0, 3, size=300)] = rng.choice([0, 64], size=300)
        k = np.concatenate([k, faces])
    outside = rng.choice(np.array([-0.25, 1.5, -1.0], dtype=np.float32), size=(64, D))
    return np.concatenate([(k / 64.0).astype(np.float32), outside])


@pytest.mark.gpu
@pytest.mark.parametrize("D,dense", [(3, False), (2, False), (3, True)])
def test_exact_lattice(D, dense):
    """Integer scales 3, 7, 15, 31, 63 and x = k / 64: every pos is exact in float32 and every weight a dyadic rational, so the
    discrete rules (cell, corner, dense index, hash, modulo, the wrap of negative cells) are compared bit for bit."""
    lv, olv = _grid(D, 5, 2, 9, 4, 2.0, dense)
    assert [float(s) for s in olv.scales] == [3.0, 7.0, 15.0, 31.0, 63.0]
    x = _lattice(D)
    assert (x == 0).any(axis=1).sum() > 20 and (x == 1).any(axis=1).sum() > 20 and x.min() == -1.0 and x.max() == 1.5
    v_out = np.random.default_rng(5).standard_normal((x.shape[0], 10)).astype(np.float32)
    _check(x, _tables(olv, 6), lv, olv, v_out, want_x=True)


@functools.lru_cache(maxsize=None)
def _random_case(F):
    lv, olv = _grid(3, 6, F, 10, 4, math.exp(math.log(96 / 4) / 5))
    assert list(olv.hashed) == [False, False, True, True, True, True] and olv.resolutions[-1] == 96
    rng = np.random.default_rng(0)
    x = rng.random((4096, 3), dtype=np.float32)
    x = x[HO.min_frac_margin(x, olv) > 1e-3]          # input construction: no frac within 1e-3 of a cell boundary
    assert 3400 < x.shape[0] < 4096
    v_out = rng.standard_normal((x.shape[0], 6 * F)).astype(np.float32)
    zero = rng.random(x.shape[0]) < 0.3
    v_out[zero] = 0.0
    table = _tables(olv, 7)
    return lv, olv, x, table, v_out, zero, HO.encode(x, table, olv, v_out, True)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 2, 4, 8])
def test_random_inputs(F):
    lv, olv, x, table, v_out, zero, ref = _random_case(F)
    _, (out, v_table, v_x) = _check(x, table, lv, olv, v_out, want_x=True, ref=ref)
    assert not v_x[zero].any() and v_x[~zero].all(axis=1).any()
    # the points whose gradient row is zero must not change v_table: the run on the other points alone gives the same, within the bound
    bound = (ref.v_table_count + 2) * U * ref.v_table_abs
    _, alone, _ = _gpu(np.ascontiguousarray(x[~zero]), table, lv, np.ascontiguousarray(v_out[~zero]))
    _within(alone, ref.v_table, bound, "v_table of the non-zero rows alone")
    _within(alone, v_table.astype(np.float64), bound, "v_table with and without the zero rows")
    assert not alone[ref.v_table_count == 0].any()


@pytest.mark.gpu
def test_contention_every_point_in_one_cell():
    """8192 points inside ONE cell of level 0: every point adds to the same 8 rows there (the in-wave sum and the atomics must lose
    nothing), and shares rows with many others at the finer levels."""
    lv, olv = _grid(3, 5, 2, 9, 4, 2.0)
    rng = np.random.default_rng(11)
    x = (0.2 + 0.25 * rng.random((8192, 3), dtype=np.float32)).astype(np.float32)
    cell, _ = HO.positions(x, olv.scales[0])
    assert (cell == 1).all()
    v_out = rng.standard_normal((8192, 10)).astype(np.float32)
    ref, _ = _check(x, _tables(olv, 12), lv, olv, v_out, want_x=True)
    assert sorted(ref.v_table_count[:64, 0][ref.v_table_count[:64, 0] > 0].tolist()) == [8192] * 8
    # the same points sorted along x: long runs of one destination inside a wave
    order = np.argsort(x[:, 0], kind="stable")
    _check(np.ascontiguousarray(x[order]), _tables(olv, 12), lv, olv, np.ascontiguousarray(v_out[order]))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [0, 1, 63, 65])
def test_edge_sizes_one_level(N):
    from gspl_amd import ops
    lv, olv = _grid(3, 1, 4, 9, 4, 2.0)
    rng = np.random.default_rng(N)
    x = rng.random((N, 3), dtype=np.float32)
    v_out = rng.standard_normal((N, 4)).astype(np.float32)
    table = _tables(olv, 2)
    ref, (out, v_table, _) = _check(x, table, lv, olv, v_out, want_x=True)
    assert out.shape == (N, 4)
    # v_table ACCUMULATES: a second backward into the same buffer gives the gradient of the points taken twice
    xd, td, vd = torch.from_numpy(x).to(DEV), torch.from_numpy(table).to(DEV), torch.from_numpy(v_out).to(DEV)
    buffer = torch.zeros_like(td)
    ops.hashgrid_backward(xd, td, lv, vd, buffer)
    ops.hashgrid_backward(xd, td, lv, vd, buffer)
    twice = HO.encode(np.concatenate([x, x]), table, olv, np.concatenate([v_out, v_out]))
    _within(buffer.cpu().numpy(), twice.v_table, (twice.v_table_count + 2) * U * twice.v_table_abs, "v_table after two calls")


@pytest.mark.gpu
def test_autograd_layouts_and_refusals():
    from gspl_amd import ops
    lv, olv = _grid(3, 5, 2, 9, 4, 2.0)
    rng = np.random.default_rng(21)
    x, table = rng.random((300, 3), dtype=np.float32), _tables(olv, 22)
    v_out = rng.standard_normal((300, 10)).astype(np.float32)
    ref = HO.encode(x, table, olv, v_out, True)
    td = torch.from_numpy(table).to(DEV).requires_grad_(True)
    wide = torch.zeros((300, 5), device=DEV)
    wide[:, 1:4] = torch.from_numpy(x).to(DEV)
    xs = wide[:, 1:4]                                    # not contiguous: copied
    assert not xs.is_contiguous()
    out = ops.hashgrid_encode(xs, td, lv)
    out.backward(torch.from_numpy(v_out).to(DEV))
    _within(out.detach().cpu().numpy(), ref.out, 8 * U * ref.out_abs, "out")
    _within(td.grad.cpu().numpy(), ref.v_table, (ref.v_table_count + 2) * U * ref.v_table_abs, "table.grad")
    assert wide.grad is None
    # the gradient for x only when x asks for it; a flat table gets a flat gradient
    xg = torch.from_numpy(x).to(DEV).requires_grad_(True)
    flat = td.detach().reshape(-1).requires_grad_(True)
    ops.hashgrid_encode(xg, flat, lv).backward(torch.from_numpy(v_out).to(DEV))
    _within(xg.grad.cpu().numpy(), ref.v_x, 8 * U * ref.v_x_abs, "x.grad")
    assert flat.grad.shape == flat.shape
    with pytest.raises(RuntimeError, match="x must be float32"):
        ops.hashgrid_encode(xg.detach().double(), td, lv)
    with pytest.raises(RuntimeError, match="table must be float32"):
        ops.hashgrid_encode(xg.detach(), td.detach().double(), lv)
    with pytest.raises(ValueError, match="x must be"):
        ops.hashgrid_encode(xg.detach()[:, :2], td, lv)
    with pytest.raises(ValueError, match="table must be"):
        ops.hashgrid_encode(xg.detach(), td.detach()[:-1], lv)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 4])
def test_guard_bands_stay_intact(F):
    """out and v_table sit between poisoned bands inside one plain tensor; forward and backward leave the bands as they were."""
    from gspl_amd import ops
    lv, olv = _grid(3, 5, F, 9, 4, 2.0)
    N, band = 333, 1024
    n_out, n_table = N * lv.n_output_dims, lv.n_params
    pad = (-n_out) % 4                                   # keeps the table's slot on a 16-byte boundary
    arena = torch.full((band + n_out + pad + band + n_table + band,), float("nan"), device=DEV)
    poison = torch.tensor(0x7FC0DEAD, dtype=torch.int32, device=DEV)
    arena.view(torch.int32).fill_(poison)
    out = arena[band:band + n_out].view(N, lv.n_output_dims)
    start = band + n_out + pad + band
    v_table = arena[start:start + n_table]
    v_table.zero_()
    rng = np.random.default_rng(31)
    x = torch.from_numpy(rng.random((N, 3), dtype=np.float32) * 3 - 1).to(DEV)          # inside and outside [0, 1]
    table = torch.from_numpy(_tables(olv, 32)).to(DEV)
    ops.hashgrid_forward(x, table, lv, out=out)
    ops.hashgrid_backward(x, table, lv, torch.from_numpy(rng.standard_normal((N, lv.n_output_dims)).astype(np.float32)).to(DEV), v_table, True)
    torch.cuda.synchronize()
    words = arena.view(torch.int32)
    for lo, hi in ((0, band), (band + n_out, start), (start + n_table, arena.numel())):
        assert bool((words[lo:hi] == poison).all()), f"the band [{lo}, {hi}) was written"
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(v_table).all()) and bool(v_table.any())

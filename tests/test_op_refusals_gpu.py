"""The refusals of the route ops that need a device tensor and that no other test covers, and one accepted call per module: a caller's
buffer comes back as the same object, a missing one is allocated with the documented shape and dtype.  Every refusal here is raised in
Python before any launch; every other call is a valid one on 5 to 8 rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32, f64, i64 = torch.float32, torch.float64, torch.int64


def Z(*shape, dtype=f32, device=DEV):
    return torch.zeros(*shape, dtype=dtype, device=device)


def R(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.fixture(scope="module")
def ops():
    from gspl_amd import ops
    return ops


@pytest.fixture(scope="module")
def hashgrid(ops):
    levels = ops.hashgrid_levels(3, 2, 2, 8, 4, 1.5)
    return levels, R(5, 3), ops.hashgrid_table(levels, device=DEV)


@pytest.fixture(scope="module")
def hexplane(ops):
    layout = ops.hexplane_layout([3, 4, 5, 2], [1], 8)
    return layout, R(5, 3), R(layout.total, 8, seed=1), ops.hexplane_box(np.array([[1.0] * 3, [-1.0] * 3], np.float32))


@pytest.fixture(scope="module")
def mask_tables():
    return R(5, 7, 16), R(6, 16, seed=1), R(8, 16, seed=2), R(16, seed=3), R(1, seed=4)


def _select(P=4, L=3):
    seg_start = (torch.arange(L * P + 1, dtype=i64) * 2).to(DEV)
    return dict(seg_start=seg_start, camera_center=Z(3), transform=torch.eye(3, device=DEV), box_min=R(P, 2), box_max=R(P, 2, seed=1) + 1,
                thresholds=torch.tensor([1.0, 2.0], device=DEV), prev_lod=Z(P, dtype=torch.int8), prev_visible=torch.ones(P, dtype=torch.bool, device=DEV))


def _glossy(N=6):
    return 1, R(N, 3), Z(3), R(N, 1, 1, seed=1), R(N, 3, 1, seed=2)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_a_misaligned_table_is_refused(ops, hashgrid, hexplane, mask_tables):
    levels, x, table = hashgrid
    with pytest.raises(ValueError, match="hashgrid_encode: table must be aligned to 16 bytes"):
        ops.hashgrid_encode(x, Z(levels.n_params + 1)[1:], levels)
    layout, x, table, _ = hexplane
    with pytest.raises(ValueError, match="hexplane_encode: table must be aligned to 16 bytes"):
        ops.hexplane_encode(x, 0.5, Z(layout.n_params + 1)[1:], np.array([[1.0] * 3, [-1.0] * 3], np.float32), layout)
    G, A, B, w2, b2 = mask_tables
    with pytest.raises(ValueError, match="spotless_mask: B must be aligned to 16 bytes"):
        ops.spotless_mask(G, A, Z(8 * 16 + 1)[1:].view(8, 16), w2, b2)


def test_a_non_contiguous_input_is_refused(ops):
    a = _select()
    with pytest.raises(RuntimeError, match="lod_select: box_min must be contiguous"):
        ops.lod_select(*{**a, "box_min": Z(4, 4)[:, ::2]}.values())
    with pytest.raises(RuntimeError, match="scales.*contiguous"):
        ops.compute_relocation(R(6), Z(6, 6)[:, ::2], torch.ones(6, dtype=i64, device=DEV), Z(3, 3))
    with pytest.raises(RuntimeError, match="opacities.*contiguous"):
        ops.mcmc_regularization(Z(6, 2)[:, 0], Z(6, 3), 1.0, 1.0, raw=True)


@pytest.mark.parametrize("bad", ["shape", "dtype"])
def test_a_wrong_buffer_is_refused(ops, hashgrid, hexplane, bad):
    def buffer(*shape, dtype=f32):
        return Z(*shape[:-1], shape[-1] + 1, dtype=dtype) if bad == "shape" else Z(*shape, dtype=f64 if dtype == f32 else torch.int32)

    with pytest.raises(ValueError, match="sh_view_opacities_forward: out must be"):
        ops.sh_view_opacities_forward(*_glossy(), out=buffer(6))
    with pytest.raises(ValueError, match="lod_select: lod must be"):
        ops.lod_select(*_select().values(), lod=buffer(4, dtype=torch.int8))
    layout, x, table, box = hexplane
    with pytest.raises(ValueError, match="hexplane_backward: v_x must be"):
        ops.hexplane_backward(x, 0.5, table, box, layout, Z(5, layout.n_output_dims), None, False, buffer(5, 3))
    levels, x, table = hashgrid
    with pytest.raises(ValueError, match="hashgrid_forward: out must be"):
        ops.hashgrid_forward(x, table, levels, out=buffer(5, levels.n_output_dims))


def test_tensors_on_two_devices_are_refused(ops, hashgrid):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    levels, x, table = hashgrid
    with pytest.raises(RuntimeError, match="hashgrid_encode: table is on cuda:1, x on cuda:0"):
        ops.hashgrid_encode(x, table.to("cuda:1"), levels)
    with pytest.raises(RuntimeError, match="sh_view_opacities: opacity_dc is on cuda:1, means on cuda:0"):
        degree, means, centre, dc, rest = _glossy()
        ops.sh_view_opacities(degree, means, centre, dc.to("cuda:1"), rest)


# ---- accepted calls: what comes back -------------------------------------------------------------------------------------------------------
def _is(t, shape, dtype=f32):
    return isinstance(t, torch.Tensor) and tuple(t.shape) == tuple(shape) and t.dtype == dtype and t.device == torch.device(DEV)


def test_glossy_returns_the_callers_buffer(ops):
    out = torch.empty(6, device=DEV)
    assert ops.sh_view_opacities_forward(*_glossy(), out=out) is out
    assert _is(ops.sh_view_opacities_forward(*_glossy()), (6,))
    v_dc, v_rest = torch.empty(6, device=DEV), torch.empty(6, 3, device=DEV)
    got = ops.sh_view_opacities_backward(*_glossy(), R(6, seed=3), v_dc, v_rest)
    assert got[0] is v_dc and got[1] is v_rest
    assert _is(ops.sh_view_opacities(*_glossy()), (6,))


def test_lod_select_returns_the_callers_buffers(ops):
    lod, record = torch.empty(4, dtype=torch.int8, device=DEV), torch.empty(2, dtype=i64, device=DEV)
    got = ops.lod_select(*_select().values(), lod=lod, record=record)          # prev_visible is bool: seen as uint8
    assert got[1] is lod and got[4] is record
    assert _is(got[0], (4,)) and _is(got[2], (4,), torch.uint8) and _is(got[3], (5,), i64)


def test_hashgrid_returns_the_callers_buffer(ops, hashgrid):
    levels, x, table = hashgrid
    out = torch.empty(5, levels.n_output_dims, device=DEV)
    assert ops.hashgrid_forward(x, table, levels, out=out) is out
    assert _is(ops.hashgrid_forward(x, table, levels), (5, 4)) and torch.equal(ops.hashgrid_encode(x, table, levels), out)
    v_table = torch.zeros_like(table)
    got = ops.hashgrid_backward(x, table, levels, R(5, 4, seed=5), v_table, True)
    assert got[0] is v_table and _is(got[1], (5, 3))


def test_hexplane_returns_the_callers_buffers(ops, hexplane):
    layout, x, table, box = hexplane
    out = torch.empty(5, 8, device=DEV)
    assert ops.hexplane_forward(x, 0.5, table, box, layout, out=out) is out
    assert _is(ops.hexplane_forward(x, 0.5, table, box, layout), (5, 8))
    v_table, v_x = torch.zeros_like(table), torch.empty(5, 3, device=DEV)
    got = ops.hexplane_backward(x, 0.5, table, box, layout, R(5, 8, seed=5), v_table, False, v_x)
    assert got[0] is v_table and got[1] is v_x
    assert ops.hexplane_backward(x, 0.5, table, box, layout, R(5, 8, seed=5), None, False) == (None, None)


def test_spotless_returns_the_callers_buffers(ops, mask_tables):
    G, A, B, w2, b2 = mask_tables
    out = torch.empty(6, 8, device=DEV)
    assert ops.spotless_mask_forward(G, A, B, w2, b2, out=out) is out and _is(ops.spotless_mask_forward(G, A, B, w2, b2, (5, 9)), (5, 9))
    v_A = torch.empty_like(A)
    got = ops.spotless_mask_backward(G, A, B, w2, b2, R(6, 8, seed=6), v_A=v_A)
    assert got[1] is v_A and _is(got[0], G.shape) and _is(got[2], B.shape) and _is(got[3], (17,))
    render, gt, mask, total = R(3, 5, 7), R(3, 5, 7, seed=1), R(5, 7, seed=2), torch.empty(1, device=DEV)
    assert ops.spotless_masked_l1_forward(render, gt, mask, out=total) is total
    v_render = torch.empty_like(render)
    assert ops.spotless_masked_l1_backward(render, gt, mask, torch.ones(1, device=DEV), v_render) is v_render
    assert _is(ops.spotless_masked_l1_backward(render, gt, mask, torch.ones(1, device=DEV)), (3, 5, 7))
    err, counts, lower, upper = ops.spotless_error_stats(render, gt, torch.tensor([0.2, 0.6], device=DEV), 8)
    assert _is(err, (5, 7)) and _is(counts, (8,), torch.int32) and _is(lower, (5, 7)) and _is(upper, (5, 7))


def test_appearance_returns_the_callers_buffer(ops):
    args = (R(5, 8), [R(32, 12, seed=1) - 0.5, R(3, 32, seed=2) - 0.5], [R(32, seed=3), R(3, seed=4)], R(4, seed=5))
    out = torch.empty(5, 3, device=DEV)
    assert ops.appearance_mlp_forward(*args, out=out) is out
    assert _is(ops.appearance_mlp(*args), (5, 3))


def test_the_older_families_return_what_they_document(ops):
    a, b = ops.mcmc_regularization(R(6), R(6, 3, seed=1), 1.0, 1.0, raw=True)
    assert _is(a, ()) and _is(b, ())
    means_t, velocity, opacity_t = ops.pvg_motion(R(6, 3), R(6, 3, seed=1), R(6, seed=2), R(6, 1, seed=3) + 0.5, R(6, 1, seed=4), 0.3, 1.0)
    assert _is(means_t, (6, 3)) and _is(velocity, (6, 3)) and _is(opacity_t, (6, 1))
    assert _is(ops.cubemap_sample(R(6, 4, 4, 3), R(5, 3, seed=1) - 0.5), (5, 3))
    assert _is(ops.depth_to_normal(R(6, 7) + 1, torch.eye(3, device=DEV)), (6, 7, 3))
    assert _is(ops.bilagrid_tv(R(1, 12, 2, 3, 3)), ())
    vertices, keys = ops.marching_tetrahedra_soup(R(3, 3, 3) - 0.5, 0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert vertices.shape[0] == keys.shape[0] and vertices.shape[0] % 3 == 0 and _is(keys, keys.shape, i64) and _is(vertices, (keys.shape[0], 3))


def test_segany_and_knn_return_what_they_document(ops):
    area, cover, mean_size = ops.segany_mask_stats(R(3, 6, 7) > 0.5)
    assert _is(area, (3,), torch.int32) and _is(cover, (6, 7), torch.int32) and _is(mean_size, (6, 7))
    points = R(1, 8, 3)
    found = ops.knn_points(points, points, K=2)
    assert _is(found.dists, (1, 8, 2)) and _is(found.idx, (1, 8, 2), i64) and found.knn is None
    graph = ops.knn_graph(found.idx[0])
    assert _is(ops.smooth_features(R(8, 5, seed=1), graph), (8, 5))

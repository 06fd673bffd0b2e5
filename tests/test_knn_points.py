"""`ops.knn_points` (csrc/knn.hip, header section 19) and the `pytorch3d.ops` stand-in: oracle self-consistency and the argument
checks on the CPU, the HIP search against the fp64 brute force on the GPU.

Tolerance of the distances: that of tests/test_knn.py — relative 2e-5 of the value plus the rounding of coordinates of magnitude
|p| (1e-6 |p|^2) — applied to the SORTED distances, which do not depend on how ties are ordered.  The tie rule itself is pinned on an
integer lattice, where every d^2 is exact in float32 and the output must equal the stable-sort oracle bit for bit."""
import functools
import importlib
import sys

import numpy as np
import pytest
import torch

import knn_points_oracle as KO
from private_pool import private_memory_pool  # noqa: F401  (autouse: the tests allocate from a pool of their own)
from test_knn import _clouds

KS = (1, 3, 16)


@functools.lru_cache(maxsize=None)
def _cloud(name):
    pts = _clouds()[name]
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _self_reference(name):
    """The 16 nearest of every point of the cloud (fp64, ties by index): computed once, its leading columns serve K = 1 and 3."""
    d2, idx = KO.knn_brute(_cloud(name), _cloud(name), 16)
    d2.setflags(write=False)
    idx.setflags(write=False)
    return d2, idx


def _check(got, queries, refs, want_d2, K):
    """Assertions 1-4 of the issue for one cloud: got = (dists [P1, K], idx [P1, K]) as numpy."""
    dists, idx = got[0].astype(np.float64), got[1]
    scale = max(float(np.abs(refs).max()), float(np.abs(queries).max()))
    tol = dict(rtol=2e-5, atol=1e-6 * scale * scale)
    assert dists.shape == idx.shape == (queries.shape[0], K)
    assert (np.diff(dists, axis=1) >= 0).all(), "a row of dists is not ascending"
    np.testing.assert_allclose(dists, want_d2[:, :K], **tol)
    assert idx.min() >= 0 and idx.max() < refs.shape[0]
    found = refs.astype(np.float64)[idx]
    np.testing.assert_allclose(((queries.astype(np.float64)[:, None, :] - found) ** 2).sum(-1), dists, **tol)
    s = np.sort(idx, axis=1)
    assert (np.diff(s, axis=1) > 0).all(), "an index appears twice in a row"


def _hip(p1, p2, K, **kw):
    from gspl_amd import ops
    a = torch.from_numpy(np.array(p1)).cuda()
    b = a if p2 is p1 else torch.from_numpy(np.array(p2)).cuda()
    out = ops.knn_points(a[None], a[None] if p2 is p1 else b[None], K=K, **kw)
    return out.dists[0].cpu().numpy(), out.idx[0].cpu().numpy()


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_oracles_agree():
    for name in ("uniform", "clustered", "plane", "line", "duplicates", "outlier"):
        pts = _cloud(name)
        q = pts[:300]
        d2, idx = KO.knn_brute(q, pts, 16)
        np.testing.assert_allclose(d2, KO.knn_kdtree_d2(q, pts, 16), rtol=1e-9, atol=1e-12, err_msg=name)
        assert (np.diff(d2, axis=1) >= 0).all()
        ties = np.diff(d2, axis=1) == 0
        assert (np.diff(idx, axis=1)[ties] > 0).all(), "equal distances must come in index order"
    d2, idx = KO.knn_brute(np.zeros((2, 3)), np.array([[0.0, 0, 1], [0, 0, 2]]), 4)
    np.testing.assert_array_equal(d2, [[1, 4, 0, 0]] * 2)
    np.testing.assert_array_equal(idx, [[0, 1, 0, 0]] * 2)


def test_standin_registers_pytorch3d_ops():
    import gspl_amd  # noqa: F401
    from gspl_amd import compat, ops
    had = "pytorch3d" in sys.modules
    installed = compat.install()
    from pytorch3d.ops import knn_points
    if not had:
        assert "pytorch3d.ops" in installed or "pytorch3d.ops" in sys.modules
        assert knn_points.__name__ == "knn_points" and "gspl_amd" in sys.modules["pytorch3d.ops"].__doc__
        with pytest.raises(ImportError):
            from pytorch3d.ops import iou_box3d  # noqa: F401
        with pytest.raises(ImportError):          # (what the partition-LoD renderer imports)
            importlib.import_module("pytorch3d.ops.iou_box3d")
        with pytest.raises(RuntimeError):
            knn_points(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), K=2)          # bound late to ops.knn_points: no CPU fallback
    assert callable(ops.knn_points) and callable(ops.knn_graph) and callable(ops.smooth_features)


def test_cpu_tensor_raises():
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    with pytest.raises(RuntimeError):
        ops.knn_points(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), K=2)
    with pytest.raises(RuntimeError):
        ops.knn_graph(torch.zeros(4, 2, dtype=torch.int64))


def test_unbuilt_arguments_raise():
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    p = torch.zeros(1, 40, 3)
    with pytest.raises(NotImplementedError):
        ops.knn_points(p, p, K=33)
    with pytest.raises(NotImplementedError):
        ops.knn_points(p, p, lengths2=torch.tensor([40]), K=3)
    with pytest.raises(NotImplementedError):
        ops.knn_points(p, p, lengths1=torch.tensor([40]), K=3)
    with pytest.raises(NotImplementedError):
        ops.knn_points(torch.zeros(1, 40, 2), torch.zeros(1, 40, 2), K=3)


def test_abi_declares_section_19():
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib
    for name in ("gspl_knn_points_workspace_bytes", "gspl_knn_points", "gspl_knn_graph_workspace_bytes", "gspl_knn_graph",
                 "gspl_smooth_features_fwd", "gspl_smooth_features_bwd"):
        assert name in _lib.exported_symbols() and hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 39


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", ["uniform", "clustered", "plane", "line", "duplicates", "outlier"])
def test_self_query_matches_oracle(name, K):
    pts = _cloud(name)
    _check(_hip(pts, pts, K), pts, pts, _self_reference(name)[0], K)


@pytest.mark.gpu
def test_self_query_finds_itself():
    pts = _cloud("uniform")
    dists, idx = _hip(pts, pts, 3)
    assert (dists[:, 0] == 0).all() and (idx[:, 0] == np.arange(pts.shape[0])).all()


@pytest.mark.gpu
def test_tie_rule_on_a_lattice():
    """Coordinates 0..7 per axis, shuffled, 64 of the points twice: every d^2 is a small integer, exact in float32."""
    rng = np.random.default_rng(3)
    grid = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    pts = np.concatenate([grid, grid[rng.choice(512, 64, replace=False)]])
    pts = np.ascontiguousarray(pts[rng.permutation(pts.shape[0])])
    want_d2, want_idx = KO.knn_brute(pts, pts, 16)
    dists, idx = _hip(pts, pts, 16)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(dists, want_d2.astype(np.float32))
    again = _hip(pts, pts, 16)
    assert np.array_equal(again[0].view(np.uint32), dists.view(np.uint32)) and np.array_equal(again[1], idx)
    # a separate query tensor takes the other query order (given order instead of cell order): the same answer
    other = _hip(pts.copy(), pts, 16)
    assert np.array_equal(other[0].view(np.uint32), dists.view(np.uint32)) and np.array_equal(other[1], idx)


@pytest.mark.gpu
def test_separate_queries_outside_the_grid():
    refs = _cloud("uniform")
    q = np.random.default_rng(5).uniform(-4, 4, size=(1000, 3)).astype(np.float32)
    assert (np.abs(q).max(1) > 1.3).mean() > 0.9          # most of them lie outside the reference cloud's box
    want, _ = KO.knn_brute(q, refs, 16)
    _check(_hip(q, refs, 16), q, refs, want, 16)


@pytest.mark.gpu
def test_sampled_rows_as_queries():
    """The regulariser's shape: a sample of the cloud's own rows against the whole cloud."""
    refs = _cloud("uniform")
    rows = np.random.default_rng(6).choice(refs.shape[0], 512, replace=False)
    q = np.ascontiguousarray(refs[rows])
    want = _self_reference("uniform")[0][rows]
    got = _hip(q, refs, 16)
    _check(got, q, refs, want, 16)
    assert (got[1][:, 0] == rows).all() and (got[0][:, 0] == 0).all()


@pytest.mark.gpu
def test_largest_k():
    """K = 32: the longest per-lane list (32 KiB of LDS per block), more than one shell for most queries."""
    refs = _cloud("clustered")
    rows = np.random.default_rng(8).choice(refs.shape[0], 400, replace=False)
    q = np.ascontiguousarray(refs[rows])
    want, _ = KO.knn_brute(q, refs, 32)
    _check(_hip(q, refs, 32), q, refs, want, 32)
    pts = _cloud("uniform")[:1500]
    want, _ = KO.knn_brute(pts, pts, 32)
    _check(_hip(pts, pts, 32), pts, pts, want, 32)


@pytest.mark.gpu
def test_edges():
    from gspl_amd import ops
    dev = torch.device("cuda:0")
    refs = _cloud("uniform")
    r = torch.from_numpy(refs.copy()).to(dev)
    # no queries
    out = ops.knn_points(torch.zeros(1, 0, 3, device=dev), r[None], K=16)
    assert out.dists.shape == (1, 0, 16) and out.idx.shape == (1, 0, 16) and out.idx.dtype == torch.int64 and out.knn is None
    # fewer reference points than K: five real neighbours, then zeros
    five, q = refs[:5], refs[100:140]
    dists, idx = _hip(q, five, 16)
    want_d2, want_idx = KO.knn_brute(q, five, 16)
    assert (dists[:, 5:] == 0).all() and (idx[:, 5:] == 0).all()
    assert np.array_equal(idx[:, :5], want_idx[:, :5])
    np.testing.assert_allclose(dists[:, :5], want_d2[:, :5], rtol=2e-5, atol=1e-6 * 1.3 * 1.3)
    # no reference points at all
    out = ops.knn_points(r[None, :7], torch.zeros(1, 0, 3, device=dev), K=4, return_nn=True)
    assert not bool(out.dists.any()) and not bool(out.idx.any()) and out.knn.shape == (1, 7, 4, 3)
    # all points coincident
    same = np.full((200, 3), 0.75, dtype=np.float32)
    dists, idx = _hip(same, same, 16)
    assert (dists == 0).all() and (idx == np.arange(16)[None, :]).all()
    # one NaN reference point in 300: never returned, everything else as if it were absent
    pts = refs[:300].copy()
    pts[137] = np.nan
    keep = np.delete(np.arange(300), 137)
    want_d2, want_idx = KO.knn_brute(pts[keep], pts[keep], 16)
    dists, idx = _hip(pts, pts, 16)
    assert (idx != 137).all()
    assert np.array_equal(idx[keep], keep[want_idx])
    np.testing.assert_allclose(dists[keep], want_d2, rtol=2e-5, atol=1e-6 * 1.3 * 1.3)
    assert np.isfinite(dists).all()                       # (the NaN query's own row: terminated, zeros)
    # two clouds in one call, with the neighbours themselves
    a, b = refs[:700], refs[700:1400] * 2.0
    both = torch.from_numpy(np.stack([a, b])).to(dev)
    qs = torch.from_numpy(np.stack([refs[2000:2050], refs[2050:2100]])).to(dev)
    out = ops.knn_points(qs, both, K=3, return_nn=True)
    for i, cloud in enumerate((a, b)):
        d2, ix = KO.knn_brute(qs[i].cpu().numpy(), cloud, 3)
        assert np.array_equal(out.idx[i].cpu().numpy(), ix)
        np.testing.assert_allclose(out.dists[i].cpu().numpy(), d2, rtol=2e-5, atol=1e-6 * 2.6 * 2.6)
        assert np.array_equal(out.knn[i].cpu().numpy(), cloud[ix])


@pytest.mark.gpu
def test_gradient_flows_through_dists():
    from gspl_amd import ops
    dev = torch.device("cuda:0")
    refs = torch.from_numpy(_cloud("uniform")[:500].copy()).to(dev)
    q = torch.from_numpy(_cloud("uniform")[500:540].copy()).to(dev).requires_grad_(True)
    out = ops.knn_points(q[None], refs[None], K=4)
    plain = ops.knn_points(q.detach()[None], refs[None], K=4)
    assert torch.equal(out.idx, plain.idx) and torch.allclose(out.dists, plain.dists, rtol=1e-5, atol=1e-6)
    out.dists.sum().backward()
    want = 2 * (q.detach()[:, None, :] - refs[plain.idx[0]]).sum(1)
    assert torch.allclose(q.grad, want, rtol=1e-5, atol=1e-6)

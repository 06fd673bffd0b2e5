"""`ops.knn_graph`, `ops.smooth_features` (csrc/smooth.hip, header section 19) and `gspl_amd.segany` on the GPU, against the reference's
formula in fp64 torch (tests/knn_points_oracle.py).

Bounds are the project's own: the outputs are unit vectors and must agree within 1e-5 absolute (the pixel tolerance); the gradient of
a random linear functional within 1e-4 of |ref| + rms (the gradient tolerance); the backward must be the same bits on every run."""
import functools
import types

import numpy as np
import pytest
import torch

import gspl_amd  # noqa: F401
from gspl_amd import ops

import knn_points_oracle as KO
from private_pool import private_memory_pool  # noqa: F401  (autouse: the tests allocate from a pool of their own)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _random_map(N, K, seed):
    """A neighbour map as a search gives one: column 0 is the row itself, the rest distinct other rows."""
    rng = np.random.default_rng(seed)
    idx = np.empty((N, K), dtype=np.int64)
    for i in range(N):
        others = rng.choice(N - 1, K - 1, replace=False)
        idx[i] = np.concatenate([[i], others + (others >= i)])
    return idx


def _star_map(N=40, K=16):
    """Row 0 is referenced by every other row (an inverse list of N - 1 entries), row N - 1 by no row at all."""
    rng = np.random.default_rng(9)
    idx = np.empty((N, K), dtype=np.int64)
    for i in range(N):
        pool = np.setdiff1d(np.arange(1, N - 1), [i])
        idx[i] = np.concatenate([[0], rng.choice(pool, K - 1, replace=False)])
    idx[0, 0] = 1                                    # (row 0 does not list itself: N - 1 references exactly)
    assert (idx == 0).sum() == N - 1 and not (idx == N - 1).any()
    return idx


CASES = {
    "half": (300, 16, 32, "random", [3, 0, 9, 14, 5, 11, 6, 12]),
    "all": (300, 16, 32, "random", None),
    "odd_width": (300, 16, 5, "random", [1, 15, 2, 8, 7, 10, 4, 13]),
    "widest": (300, 16, 128, "random", [3, 0, 9, 14, 5, 11, 6, 12]),           # four float4 chunks per lane
    "ragged_float4": (300, 16, 36, "random", [3, 0, 9, 14, 5, 11, 6, 12]),     # a second chunk that only one lane of eight holds
    "ragged_scalar": (300, 16, 67, "random", None),                             # the scalar path with three chunks, the last ragged
    "star": (40, 16, 32, "star", [0, 2, 4, 6, 8, 10, 12, 14]),
    "zero_row": (300, 16, 32, "random", [3, 0, 9, 14, 5, 11, 6, 12]),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and the fp64 reference of one case, computed once."""
    N, K, D, kind, columns = CASES[name]
    rng = np.random.default_rng(17)
    idx = _random_map(N, K, 4) if kind == "random" else _star_map(N, K)
    x = rng.normal(size=(N, D)).astype(np.float32) * rng.uniform(0.1, 3.0, size=(N, 1)).astype(np.float32)
    if name == "zero_row":
        x[7] = 0.0                                    # the 1e-12 guard of the first normalisation ...
        idx[21] = 7                                   # ... and a row whose mean is exactly zero: the 1e-9 guard of the second
    w = rng.normal(size=(N, D)).astype(np.float32)
    out, grad = KO.smooth_reference_with_grad(x, idx, w, columns)
    for a in (idx, x, w, out, grad):
        a.setflags(write=False)
    return idx, x, w, out, grad, columns


def _run(name):
    idx, x, w, _, _, columns = _case(name)
    graph = ops.knn_graph(torch.from_numpy(idx.copy()).to(DEV))
    feats = torch.from_numpy(x.copy()).to(DEV).requires_grad_(True)
    out = ops.smooth_features(feats, graph, None if columns is None else torch.tensor(columns))
    (out * torch.from_numpy(w.copy()).to(DEV)).sum().backward()
    return out.detach().cpu().numpy(), feats.grad.cpu().numpy(), graph


def test_graph_is_the_sorted_inverse_adjacency():
    for idx in (_random_map(300, 16, 4), _star_map()):
        N, K = idx.shape
        g = ops.knn_graph(torch.from_numpy(idx.copy()).to(DEV))
        assert g.idx.dtype == torch.int32 and torch.equal(g.idx.cpu().long(), torch.from_numpy(idx.copy()))
        start, entries = g.row_start.cpu().numpy(), g.entries.cpu().numpy()
        flat = idx.reshape(-1)
        order = np.argsort(flat, kind="stable")          # by (j, e): e = i K + k ascending inside a row
        assert np.array_equal(start, np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=N))]))
        assert np.array_equal(entries, order)
        again = ops.knn_graph(torch.from_numpy(idx.copy()).to(DEV))
        assert torch.equal(again.entries, g.entries) and torch.equal(again.row_start, g.row_start)
    star = ops.knn_graph(torch.from_numpy(_star_map()).to(DEV))
    assert star.inverse(0).shape == (39, 2) and star.inverse(39).shape == (0, 2)
    with pytest.raises(ValueError):
        ops.knn_graph(torch.full((4, 2), 4, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("name", ["half", "all", "odd_width", "widest", "ragged_float4", "ragged_scalar", "star", "zero_row"])
def test_forward_and_gradient_match_the_reference(name):
    _, _, _, want_out, want_grad, _ = _case(name)
    out, grad, _ = _run(name)
    assert np.isfinite(out).all() and np.isfinite(grad).all()
    worst = np.abs(out - want_out).max()
    rms = np.sqrt(np.mean(want_grad * want_grad))
    rel = (np.abs(grad - want_grad) / (np.abs(want_grad) + rms)).max()
    print(f"{name}: forward max |diff| {worst:.3e}, gradient worst / (|ref| + rms) {rel:.3e}")
    assert worst <= 1e-5
    assert rel <= 1e-4


def test_backward_is_bit_reproducible():
    for name in ("half", "star"):
        a, b = _run(name), _run(name)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_argument_checks():
    idx, x, _, _, _, _ = _case("half")
    graph = ops.knn_graph(torch.from_numpy(idx.copy()).to(DEV))
    feats = torch.from_numpy(x.copy()).to(DEV)
    with pytest.raises(RuntimeError):
        ops.smooth_features(feats.cpu(), graph)
    with pytest.raises(ValueError):
        ops.smooth_features(feats[:100], graph)
    with pytest.raises(ValueError):
        ops.smooth_features(feats, graph, [16])
    with pytest.raises(NotImplementedError):
        ops.smooth_features(torch.zeros(300, 129, device=DEV), graph)


def test_feature_smoother():
    from gspl_amd.segany import HipFeatureSmoother
    pts = torch.from_numpy(np.random.default_rng(2).uniform(-1.3, 1.3, size=(600, 3)).astype(np.float32)).to(DEV)
    feats = torch.randn(600, 32, generator=torch.Generator().manual_seed(5)).to(DEV)
    sm = HipFeatureSmoother(K=16, dropout=0.5)
    # eval: all K columns of the searched map
    out = sm(feats, pts, training=False)
    graph = sm.graph
    assert sm.last_columns is None and graph.K == 16 and graph.N == 600
    idx = ops.knn_points(pts[None], pts[None], K=16).idx[0]
    assert torch.equal(graph.idx.long(), idx)
    want = KO.smooth_reference(feats.cpu(), idx.cpu(), None).numpy()
    assert np.abs(out.cpu().numpy() - want).max() <= 1e-5
    # training: int(K * dropout) columns from the given generator, the cached map
    out = sm(feats, pts, training=True, generator=torch.Generator().manual_seed(11))
    columns = torch.randperm(16, generator=torch.Generator().manual_seed(11))[:8]
    assert torch.equal(sm.last_columns, columns) and sm.graph is graph
    want = KO.smooth_reference(feats.cpu(), idx.cpu(), columns.tolist()).numpy()
    assert np.abs(out.cpu().numpy() - want).max() <= 1e-5
    # another K: the map is searched again
    sm.K = 4
    out = sm(feats, pts, training=False)
    assert sm.graph is not graph and sm.graph.K == 4 and torch.equal(sm.graph.idx.long(), idx[:, :4])
    want = KO.smooth_reference(feats.cpu(), idx[:, :4].cpu(), None).numpy()
    assert np.abs(out.cpu().numpy() - want).max() <= 1e-5
    # K <= 1: the features re-normalised
    one = HipFeatureSmoother(K=1)(feats, pts, training=True)
    assert torch.allclose(one, feats / (feats.norm(dim=-1, keepdim=True) + 1e-9)) and HipFeatureSmoother(K=1).graph is None
    with pytest.raises(AssertionError):
        HipFeatureSmoother(K=16, dropout=0.01)(feats, pts, training=True)


def test_use_hip_smoothing_feeds_the_renderer():
    from fakes import FakeCamera, FakePropertyModel
    from gspl_amd.renderers import HipGSplatContrastiveFeatureRenderer
    from gspl_amd.segany import use_hip_smoothing
    from oracle import gsplat_oracle as O
    n, W, H = 3000, 97, 65
    means, scales, quats, opac, shs = O.synthetic_scene(n, seed=11)
    model = FakePropertyModel(*[t.to(DEV) for t in (means, scales * 3, quats, opac, shs)])
    for p in model.properties.values():
        p.requires_grad_(False)                       # SegAnyGS trains features over a frozen model
    cam = FakeCamera(O.synthetic_camera(W, H, 260.0), DEV)

    class Module(torch.nn.Module):                    # the attributes of SegAnySplatting that the smoothing reads
        def __init__(self):
            super().__init__()
            self.gaussian_semantic_features = torch.nn.Parameter(torch.randn(n, 32, generator=torch.Generator().manual_seed(3)).to(DEV))
            self.models = types.SimpleNamespace(gaussian=model)
            self.smooth_K, self.smooth_dropout = 16, 0.5
            self.renderer = HipGSplatContrastiveFeatureRenderer()

        def get_processed_semantic_features(self):
            raise AssertionError("the reference's route: needs pytorch3d and gathers [N, 8, 32]")

    module = Module()
    smoother = use_hip_smoothing(module, generator=torch.Generator().manual_seed(1))
    assert module.hip_feature_smoother is smoother
    module.train()
    feats = module.get_processed_semantic_features()
    assert feats.shape == (n, 32) and smoother.last_columns.numel() == 8
    assert torch.allclose(feats.norm(dim=-1), torch.ones(n, device=DEV), atol=1e-5)
    out = module.renderer(cam, model, torch.zeros(32, device=DEV), semantic_features=feats)
    assert out["render"].shape == (32, H, W)
    out["render"].square().sum().backward()
    grad = module.gaussian_semantic_features.grad
    assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    module.eval()
    assert module.get_processed_semantic_features().shape == (n, 32) and smoother.last_columns is None

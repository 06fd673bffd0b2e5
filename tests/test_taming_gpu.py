"""`ops.positive_medians`, `ops.taming_score_accumulate_`, `ops.find_edges` (include/gspl_hip.h section 27, csrc/taming.hip) and
`gspl_amd.taming.compute_gaussian_score` on the GPU against the fp64 / integer oracle tests/taming_oracle.py, which tests/test_taming.py
pins to the reference's own run and to PIL.  Nothing here reads the reference tree.

Tolerances.  u = 2^-24, the unit roundoff of float32; the inputs are float32 values, which the oracle widens exactly.
  counts, medians     exact: the radix select returns an entry of the row, bit for bit the one the sorted oracle picks.
  score accumulate    against the oracle evaluated with the KERNEL'S OWN medians (bit-equal to the oracle's anyway).  Nonnegative
                      coefficients, so every term is >= 0 and every partial sum is bounded by the result.  One view: a term is a quotient
                      and a product (2), the nine terms meet in eight additions (8), then w's product (1), the visibility product (1,
                      exact in fact) and the accumulate (1): 13 u relative to the result (SCORE_ROUNDINGS); each further view adds its
                      accumulate (1): 15 u for three views.  The same count holds for the accumulated total because all summands are >= 0.
  edge map            the byte image exactly; the normalised map within 4 u of the fp64 oracle (e / 255, two differences, one quotient).
The GPU tests never widen these; each prints the worst fraction of its bound."""
import os

import numpy as np
import pytest
import torch

import taming_oracle as TO
from fakes import FakeCamera, FakeGaussianModel
from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
SCORE_ROUNDINGS = 2 + 8 + 1 + 1 + 1
EDGE_ROUNDINGS = 1 + 2 + 1
SIZES = [1, 2, 255, 256, 257, 70_001]          # 70 001: seventeen full workgroups of 4096 entries and a tail of 369
KINDS = ["binades", "one_binade", "half_invalid"]
NO_VALID_ROW, I32_ROW = 7, 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_taming.npz")
COEFFS = [25, 100, 5, 10, 25, 50, 10, 0.1, 50]          # the reference's defaults in the order of addition


def make_rows(N, kind, seed=0):
    """Nine rows (numpy): row 3 int32, row 7 without a valid entry (zeros, negatives, NaN); the others by `kind`:
    binades: 2^U[-15, 15] x U[1, 2), thirty binades;  one_binade: all inside [1, 2), the first digit pass separates nothing;
    half_invalid: the binades rows with half of the entries replaced by 0, negatives and NaN."""
    rng = np.random.default_rng(1000 * N + 7 * KINDS.index(kind) + seed)
    rows = []
    for r in range(9):
        if r == I32_ROW:
            v = rng.integers(-3, 60, size=N).astype(np.int32) if kind != "one_binade" else rng.integers(1, 3, size=N).astype(np.int32)
            if kind == "half_invalid":
                v[rng.random(N) < 0.5] = 0
        elif r == NO_VALID_ROW:
            v = rng.choice(np.array([0.0, -1.5, np.nan, -0.0, -np.inf], dtype=np.float32), size=N)
        else:
            if kind == "one_binade":
                v = (1.0 + rng.random(N)).astype(np.float32)
                v[v >= 2.0] = np.float32(1.5)
            else:
                v = (np.exp2(rng.integers(-15, 15, size=N).astype(np.float64)) * (1.0 + rng.random(N))).astype(np.float32)
            if kind == "half_invalid":
                bad = rng.random(N) < 0.5
                v[bad] = rng.choice(np.array([0.0, -2.0, np.nan], dtype=np.float32), size=int(bad.sum()))
        rows.append(v)
    return rows


def to_dev(rows):
    return [torch.from_numpy(r.copy()).to(DEV) for r in rows]


def raw_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", SIZES)
def test_medians_are_exact(N, kind):
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    rows = make_rows(N, kind)
    dev = to_dev(rows)
    counts, medians = ops.positive_medians(dev)
    again_c, again_m = ops.positive_medians(dev)
    want_c, want_m = TO.positive_medians(rows)
    got_c, got_m = counts.cpu().numpy(), medians.cpu().numpy()
    assert counts.dtype == torch.int32 and medians.dtype == torch.float32 and counts.is_cuda
    assert np.array_equal(got_c, want_c), (got_c, want_c)
    assert np.array_equal(raw_bits(got_m), raw_bits(want_m)), (got_m, want_m)
    assert got_c[NO_VALID_ROW] == 0 and np.isnan(got_m[NO_VALID_ROW])
    assert np.array_equal(again_c.cpu().numpy(), got_c) and np.array_equal(raw_bits(again_m.cpu().numpy()), raw_bits(got_m))
    for d, r in zip(dev, rows):
        assert np.array_equal(raw_bits(d.cpu().numpy()), raw_bits(r))          # the inputs are not modified


def test_medians_of_edge_rows_and_unaligned_views():
    """The golden rows of tests/test_taming.py (n = 1, n = 2, ties, +inf, subnormals, an int32 row with INT_MAX, no valid entry) one row at a
    time, and rows that are views starting 4 bytes into an allocation (no 16-byte loads)."""
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    ref = dict(np.load(GOLDEN))
    for name in ("n1", "n2_lower", "even", "odd", "all_equal", "ties", "none_valid", "with_inf", "subnormals", "i32"):
        row = ref[f"row/{name}"]
        c, m = ops.positive_medians([torch.from_numpy(row).to(DEV)])
        n, want = TO.positive_median(row)
        assert int(c[0]) == n, name
        assert raw_bits(m.cpu().numpy())[0] == raw_bits(np.array([want], dtype=np.float32))[0], (name, m, want)
    rows = make_rows(5001, "binades", seed=3)
    shifted = [torch.from_numpy(np.concatenate([r[:1], r])).to(DEV)[1:] for r in rows]
    assert all(t.data_ptr() % 16 == 4 for t in shifted)
    c, m = ops.positive_medians(shifted)
    want_c, want_m = TO.positive_medians(rows)
    assert np.array_equal(c.cpu().numpy(), want_c) and np.array_equal(raw_bits(m.cpu().numpy()), raw_bits(want_m))


def score_fraction(got, base, rows, medians, counts, w, visible, roundings):
    """max |(got - base) - oracle| / (roundings u |oracle|): with nonnegative terms the bound is relative to the oracle's value; rows
    where the oracle is exactly 0 must be exact."""
    value, _ = TO.score(rows, COEFFS, medians, w, visible, counts)
    err = np.abs(got.astype(np.float64) - base.astype(np.float64) - value)
    assert np.all(err[value == 0] == 0)
    return float(np.max(np.where(value == 0, 0.0, err / np.maximum(roundings * U * np.abs(value), 1e-300))))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", SIZES)
def test_score_accumulate_against_the_oracle(N, kind):
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    rng = np.random.default_rng(N + 31)
    rows = make_rows(N, kind)
    dead = rng.random(N) < 0.1                       # Gaussians whose every entry is invalid
    for r, v in enumerate(rows):
        v[dead] = 0
    visible = rng.random(N) < 0.75
    dev = to_dev(rows)
    counts, medians = ops.positive_medians(dev)
    w = np.float32(50 * 0.0423)
    imp = torch.zeros(N, device=DEV)
    out = ops.taming_score_accumulate_(imp, dev, COEFFS, counts, medians, torch.tensor(w, device=DEV), torch.from_numpy(visible).to(DEV), n_first=5)
    assert out is imp
    got = imp.cpu().numpy()
    m, c = medians.cpu().numpy(), counts.cpu().numpy()
    worst = score_fraction(got, np.zeros(N, np.float32), rows, m, c, w, visible, SCORE_ROUNDINGS)
    print(f"score accumulate N={N} {kind}: worst fraction of {SCORE_ROUNDINGS} u: {worst:.3f}")
    assert worst <= 1.0
    assert not got[~visible].any() and not got[dead].any()
    assert kind != "binades" or N < 3 or got[visible & ~dead].min() > 0
    # two runs give the same bits
    imp2 = torch.zeros(N, device=DEV)
    ops.taming_score_accumulate_(imp2, dev, COEFFS, counts, medians, torch.tensor(w, device=DEV), torch.from_numpy(visible).to(DEV).view(torch.uint8), n_first=5)
    assert torch.equal(imp, imp2)


def test_score_accumulates_over_three_calls_and_leaves_rows_alone():
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    N = 70_001
    rng = np.random.default_rng(9)
    start = rng.random(N).astype(np.float32)
    imp = torch.from_numpy(start.copy()).to(DEV)
    total = np.zeros(N, np.float64)
    never = rng.random(N) < 0.05                      # invisible in every view
    dead = rng.random(N) < 0.05                       # every entry invalid in every view
    for view in range(3):
        rows = make_rows(N, "binades" if view != 1 else "half_invalid", seed=view)
        for v in rows:
            v[dead] = 0
        visible = (rng.random(N) < 0.7) & ~never
        dev = to_dev(rows)
        counts, medians = ops.positive_medians(dev)
        w = np.float32(0.9 + view)
        ops.taming_score_accumulate_(imp, dev, COEFFS, counts, medians, torch.tensor([w], device=DEV), torch.from_numpy(visible).to(DEV))
        value, _ = TO.score(rows, COEFFS, medians.cpu().numpy(), w, visible, counts.cpu().numpy())
        total += value
    got = imp.cpu().numpy()
    assert np.array_equal(got[never], start[never]) and np.array_equal(got[dead], start[dead])
    # relative to the accumulated total INCLUDING the start value, all summands >= 0: 13 u for the first view's sum, + 1 per further view
    want = start.astype(np.float64) + total
    err = np.abs(got.astype(np.float64) - want)
    worst = float(np.max(err / ((SCORE_ROUNDINGS + 2) * U * want)))
    print(f"three views: worst fraction of {SCORE_ROUNDINGS + 2} u: {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["levels", "1x1", "1x7", "2x5", "3x3", "floats"])
def test_edges_equal_pil_and_the_oracle(name):
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    ref = dict(np.load(GOLDEN))
    img = ref["imgf/floats"] if name == "floats" else ref[f"img/{name}"]
    e = TO.edge_bytes_fast(img)
    assert np.array_equal(e, ref[f"pil_edges/{name}"].astype(np.int64))
    got = ops.find_edges(torch.from_numpy(img).to(DEV))
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == img.shape[1:]
    g = got.cpu().numpy()
    if e.max() == e.min():
        assert np.isnan(g).all()
        return
    # the byte image back out of the normalised map: e = min + round(g (max - min)), exact since |error| << 1 / 255
    back = np.rint(g.astype(np.float64) * (e.max() - e.min())).astype(np.int64) + e.min()
    assert np.array_equal(back, e)
    want = TO.normalised_edges(e)
    err = np.abs(g.astype(np.float64) - want)
    worst = float(np.max(np.where(err == 0, 0.0, err / np.maximum(EDGE_ROUNDINGS * U * np.abs(want), 1e-300))))
    print(f"edge map {name}: worst fraction of {EDGE_ROUNDINGS} u: {worst:.3f}")
    assert worst <= 1.0
    assert torch.equal(got.cpu(), ops.find_edges(torch.from_numpy(img)))          # and bit-equal to the CPU path
    if img.dtype == np.uint8:
        assert torch.equal(ops.find_edges((torch.from_numpy(img).float() / 255.).to(DEV)), got)          # uint8 and float inputs agree


def test_edges_of_a_frame_of_many_workgroups_and_a_constant_one():
    """200 x 333 pixels: seventeen workgroups of 4096 pixels and a tail, so that the min / max really is folded across workgroups."""
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    rng = np.random.default_rng(4)
    img = rng.integers(40, 200, size=(3, 200, 333)).astype(np.uint8)
    img[:, 150, 300] = 255
    img[:, 149:152, 299:302:2] = 0
    got = ops.find_edges(torch.from_numpy(img).to(DEV))
    assert torch.equal(got.cpu(), ops.find_edges(torch.from_numpy(img)))
    e = TO.edge_bytes_fast(img)
    assert e.min() == 0 and e.max() == 255 and float(got.min()) == 0.0 and float(got.max()) == 1.0
    assert bool(torch.isnan(ops.find_edges(torch.zeros((3, 70, 90), dtype=torch.uint8, device=DEV))).all())


class _HostReads:
    """Counts `torch.cuda.synchronize`, `Tensor.item`, `.cpu`, `.tolist`, `.numpy` and `.nonzero` while `on` is set."""
    NAMES = ("item", "cpu", "tolist", "numpy", "nonzero", "__bool__", "__int__", "__float__")

    def __init__(self, monkeypatch):
        self.on, self.count = False, 0
        for name in self.NAMES:
            monkeypatch.setattr(torch.Tensor, name, self._wrap(getattr(torch.Tensor, name)))
        monkeypatch.setattr(torch.cuda, "synchronize", self._wrap(torch.cuda.synchronize))

    def _wrap(self, fn):
        def counted(*a, **k):
            if self.on:
                self.count += 1
            return fn(*a, **k)
        return counted


def test_compute_gaussian_score_end_to_end(monkeypatch):
    """N = 2 000 Gaussians, a 64 x 48 frame, 3 views through HipGSplatV1Renderer.  The ops record what they were given; the same function
    then runs again with the renderer and `rasterize_to_weights` REPLAYING the first run's outputs (the compositing sums are float atomics:
    a second rendering differs in the last bits, and a median moves with them) and the medians and the accumulate replaced by the fp64
    oracle.  Bound: 13 u for the first view + 1 per further view, relative to the oracle's total (all terms >= 0).  After the renderer
    returns nothing in the loop waits for the device."""
    import gspl_amd  # noqa: F401
    from gspl_amd import ops, synthetic, taming
    from gspl_amd.renderers import HipGSplatV1Renderer
    N, W, H, VIEWS = 2000, 64, 48, 3
    means, scales, quats, opac, shs = synthetic.scene(N, seed=7)
    model = FakeGaussianModel(*[t.to(DEV) for t in (means, scales * 6, quats, opac, shs)])
    cams = [FakeCamera(c, DEV) for c in synthetic.camera_set(W, H, 60.0, count=VIEWS, distance=4.0)]
    g = torch.Generator().manual_seed(1)
    images = [(torch.rand(3, H, W, generator=g) * 255).to(torch.uint8) for _ in range(VIEWS)]
    sample = [(cam, ("view", img.to(DEV), None), None) for cam, img in zip(cams, images)]
    edges = taming.edge_maps(sample)
    for e, img in zip(edges, images):
        assert e.is_cuda and torch.equal(e.cpu(), ops.find_edges(img))
    grads = (torch.rand(N, generator=g) * 1e-3 * (torch.rand(N, generator=g) < 0.8)).to(DEV)
    bg = torch.zeros(3, device=DEV)
    coeffs = taming.ScoreCoefficients()
    renderer = HipGSplatV1Renderer().instantiate()

    reads = _HostReads(monkeypatch)
    rendered, weights, calls = [], [], []

    class Recording:
        def training_forward(self, *a, **k):
            reads.on = False
            out = renderer.training_forward(*a, **k)
            rendered.append(out)
            reads.on = True
            return out

    def recording_weights(**k):
        out = taming.rasterize_to_weights(**k)
        weights.append(tuple(t.clone() for t in out))
        return out

    def recording_medians(rows):
        calls.append("medians")
        return ops.positive_medians(rows)

    def recording_accumulate(*a, **k):
        calls.append("accumulate")
        return ops.taming_score_accumulate_(*a, **k)

    torch.cuda.synchronize()
    score = taming.compute_gaussian_score(model, Recording(), 0, grads, sample, edges, bg, coeffs, 0.2, medians_op=recording_medians,
                                          accumulate_op=recording_accumulate, weights_op=recording_weights)
    reads.on = False
    assert reads.count == 0, f"{reads.count} host read(s) in the loop after the renderer returned"
    assert calls == ["medians", "accumulate"] * VIEWS and len(rendered) == VIEWS
    torch.cuda.synchronize()

    total = np.zeros(N, np.float64)
    replay_r, replay_w = iter(rendered), iter(weights)

    class Replaying:
        def training_forward(self, *a, **k):
            return next(replay_r)

    def oracle_medians(rows):
        c, m = TO.positive_medians([r.cpu().numpy() for r in rows])
        return torch.from_numpy(c), torch.from_numpy(m)

    def oracle_accumulate(importance, rows, c, counts, medians, w, visible, n_first):
        assert n_first == 5 and list(c) == COEFFS
        value, _ = TO.score([r.cpu().numpy() for r in rows], c, medians.numpy(), np.float32(w.cpu().numpy()), visible.cpu().numpy(), counts.numpy())
        total[:] += value
        return importance

    taming.compute_gaussian_score(model, Replaying(), 0, grads, sample, edges, bg, coeffs, 0.2, medians_op=oracle_medians,
                                  accumulate_op=oracle_accumulate, weights_op=lambda **k: next(replay_w))
    got = score.cpu().numpy().astype(np.float64)
    seen = np.zeros(N, bool)
    for out in rendered:
        seen |= out["visibility_filter"].cpu().numpy()
    assert seen.sum() > N // 2 and np.all(got[~seen] == 0) and np.all(total[~seen] == 0) and np.all(got[seen] > 0)
    err = np.abs(got - total)
    worst = float(np.max(np.where(total == 0, err, err / np.maximum((SCORE_ROUNDINGS + VIEWS - 1) * U * total, 1e-300))))
    print(f"compute_gaussian_score: {int(seen.sum())} of {N} Gaussians scored, worst fraction of {SCORE_ROUNDINGS + VIEWS - 1} u: {worst:.3f}")
    assert worst <= 1.0

"""The Taming-3DGS route without a GPU: `gspl_amd.taming.count_array`, `loss_map` and the CPU paths of `ops.positive_medians`,
`ops.taming_score_accumulate_` and `ops.find_edges`, and the fp64 / integer oracle tests/taming_oracle.py, all against
tests/golden/ref_taming.npz — the reference's own `Taming3DGSUtils` (unedited) and PIL's own `convert('L')` / `FIND_EDGES`, recorded by
tests/golden/make_taming_golden.py where the reference tree is present.  Nothing here reads that tree.

Tolerances.  u = 2^-24, the unit roundoff of float32.
  medians, counts, count_array, the byte images: exact.
  a normalised row c * (v / median): bit-equal to the reference's `normalize` (the same two float32 operations).
  the normalised edge map against the fp64 oracle evaluated from the INTEGER edge values: 4 u relative to the result — x = e / 255, the
      two differences x - min and max - min, and the quotient, one rounding each.  The test counts them and prints the worst fraction."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import taming_oracle as TO

import gspl_amd  # noqa: F401
from gspl_amd import ops, taming

U = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_taming.npz")
ROWS = ("n1", "n2_lower", "even", "odd", "all_equal", "ties", "none_valid", "with_inf", "subnormals", "i32")
IMAGES = ("levels", "1x1", "1x7", "2x5", "3x3")


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(GOLDEN))


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def test_count_array_equals_the_reference(ref):
    at = 0
    assert len(ref["count/len"]) >= 5 and set(ref["count/mode"].tolist()) == {0, 1}
    for cfg, mode, n in zip(ref["count/cfg"], ref["count/mode"], ref["count/len"]):
        start, mult, until, frm, interval = cfg
        mult = float(mult) if mode == 0 else int(mult)
        args = (int(start), mult, int(until), int(frm), int(interval), "multiplier" if mode == 0 else "final_count")
        want = ref["count/values"][at:at + n].tolist()
        at += n
        assert taming.count_array(*args) == want and TO.count_array(*args) == want, args
        assert all(isinstance(v, int) for v in taming.count_array(*args))
    # a budget below the start count: nothing to add, the curve stays at the start count
    assert set(taming.count_array(100000, 60000, 15000, 500, 100, "final_count")) == {100000}
    with pytest.raises(ValueError):
        taming.count_array(10, 2, 100, 0, 10, "other")


@pytest.mark.parametrize("name", ROWS)
def test_median_equals_torch_median_of_the_positive_entries(ref, name):
    row = ref[f"row/{name}"]
    before = row.copy()
    t = torch.from_numpy(row)
    counts, medians = ops.positive_medians([t])
    n, m = TO.positive_median(row)
    assert counts.dtype == torch.int32 and medians.dtype == torch.float32
    assert int(counts[0]) == n
    if name == "none_valid":
        assert n == 0 and np.isnan(m) and bool(torch.isnan(medians[0])) and f"median/{name}" not in ref
    else:
        want = ref[f"median/{name}"]
        assert bits(medians.numpy())[0] == bits(want)[0] == bits(m), (name, medians, want, m)
    assert np.array_equal(bits(row) if row.dtype == np.float32 else row, bits(before) if row.dtype == np.float32 else before)   # untouched
    expected = {"n1": 1, "n2_lower": 2, "even": 40, "odd": None, "all_equal": 17, "ties": 9, "none_valid": 0, "with_inf": 5, "subnormals": 4, "i32": 6}[name]
    assert expected is None or n == expected
    if name == "n2_lower":
        assert float(medians[0]) == 2.0
    if name == "with_inf":
        assert float(medians[0]) == float("inf")
    if name == "ties":
        assert float(medians[0]) == 2.0
    if name == "subnormals":
        assert 0 < float(medians[0]) < 1.2e-38


def test_all_rows_at_once_and_the_callers_buffers(ref):
    by_len = {}
    for name in ROWS:
        by_len.setdefault(len(ref[f"row/{name}"]), []).append(name)
    names = max(by_len.values(), key=len)
    rows = [torch.from_numpy(ref[f"row/{n}"]) for n in names]
    counts, medians = torch.zeros(len(rows), dtype=torch.int32), torch.zeros(len(rows))
    c, m = ops.positive_medians(rows, counts=counts, medians=medians)
    assert c is counts and m is medians
    wc, wm = TO.positive_medians([ref[f"row/{n}"] for n in names])
    assert np.array_equal(counts.numpy(), wc) and np.array_equal(bits(medians.numpy()), bits(wm))


@pytest.mark.parametrize("name", ROWS)
def test_normalised_row_equals_the_reference_normalize(ref, name):
    """One row, multiplier 7.5, w = 1, everything visible, importance 0: the accumulate IS `normalize`."""
    row = torch.from_numpy(ref[f"row/{name}"])
    counts, medians = ops.positive_medians([row])
    imp = torch.zeros(row.numel())
    out = ops.taming_score_accumulate_(imp, [row], [7.5], counts, medians, torch.tensor(1.0), torch.ones(row.numel(), dtype=torch.bool), n_first=1)
    assert out is imp
    want = ref[f"norm/{name}"]
    assert np.array_equal(bits(imp.numpy()), bits(want)), (name, imp, want)
    if name == "none_valid":
        assert not imp.any()


def test_score_association_and_oracle(ref):
    """Nine rows in the reference's order of addition: the CPU path equals the reference's expression written out in torch (bitwise),
    and the fp64 oracle within 13 u of the terms' magnitudes (the count of tests/test_taming_gpu.py)."""
    g = torch.Generator().manual_seed(5)
    N = 257
    rows = [torch.rand(N, generator=g) * 10 ** float(torch.randint(-3, 4, (1,), generator=g)) for _ in range(9)]
    rows[3] = torch.randint(-2, 40, (N,), generator=g, dtype=torch.int32)
    for r in rows[:3] + rows[4:]:
        r[torch.rand(N, generator=g) < 0.2] = 0.0
    rows[6][5] = float("nan")
    visible = torch.rand(N, generator=g) < 0.7
    coeffs = taming.score_coefficients(taming.ScoreCoefficients())
    assert coeffs == [25, 100, 5, 10, 25, 50, 10, 0.1, 50]
    counts, medians = ops.positive_medians(rows)
    w = torch.tensor(50 * 0.0371, dtype=torch.float32)
    imp0 = torch.rand(N, generator=g)
    imp = ops.taming_score_accumulate_(imp0.clone(), rows, coeffs, counts, medians, w, visible, n_first=5)

    def normalize(c, v):      # the reference's, :455-465
        v = v.clone()
        v[v.isnan()] = 0
        ok = v > 0
        ret = torch.zeros_like(v, dtype=torch.float32)
        val = v[ok].to(torch.float32)
        ret[ok] = c * (val / torch.median(val))
        return ret
    t = [normalize(c, r) for c, r in zip(coeffs, rows)]
    g_imp = t[0] + t[1] + t[2] + t[3] + t[4]
    p_imp = t[5] + t[6] + t[7] + t[8]
    want = imp0 + w * (p_imp + g_imp) * visible
    assert torch.equal(imp, want)
    assert torch.equal(imp[~visible], imp0[~visible])
    value, mag = TO.score([r.numpy() for r in rows], coeffs, medians.numpy(), float(w), visible.numpy(), counts.numpy())
    err = np.abs((imp - imp0).double().numpy() - value)
    bound = 13 * U * mag + 2 * U * np.abs(imp.double().numpy())          # + the accumulate's own rounding, relative to the result
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"score CPU path against the fp64 oracle: worst fraction of the bound {worst:.3f}")
    assert worst <= 1.0


def test_loss_map_equals_the_reference(ref):
    out = taming.loss_map(torch.from_numpy(ref["lossmap/render"]), torch.from_numpy(ref["lossmap/gt"]), taming.ScoreCoefficients(),
                          torch.from_numpy(ref["lossmap/edges"]))
    assert np.array_equal(bits(out.numpy()), bits(ref["lossmap/out"]))
    want = TO.loss_map(ref["lossmap/render"], ref["lossmap/gt"], 50, 50, ref["lossmap/edges"])
    assert np.allclose(out.numpy(), want, rtol=0, atol=1e-4)


@pytest.mark.parametrize("name", IMAGES)
def test_edge_bytes_equal_pil(ref, name):
    img = ref[f"img/{name}"]
    if name == "levels":
        assert all(len(np.unique(img[c])) == 256 for c in range(3))
    assert np.array_equal(TO.grey(img), ref[f"pil_l/{name}"])
    want = ref[f"pil_edges/{name}"].astype(np.int64)
    assert np.array_equal(TO.edge_bytes(img), want) and np.array_equal(TO.edge_bytes_fast(img), want)
    assert np.array_equal(ops.taming.edge_bytes(torch.from_numpy(img)).numpy(), want)
    assert np.array_equal(ops.taming.edge_bytes(torch.from_numpy(img).float() / 255.).numpy(), want)
    # ... and the reference's get_edges is those bytes / 255
    assert np.array_equal(bits(ref[f"edges/{name}"]), bits(want.astype(np.float32) / np.float32(255)))


def test_float_images_are_quantised_as_topilimage_does(ref):
    img = ref["imgf/floats"]
    want = ref["pil_edges/floats"].astype(np.int64)
    assert np.array_equal(TO.edge_bytes(img), want)
    assert np.array_equal(ops.taming.edge_bytes(torch.from_numpy(img)).numpy(), want)
    assert np.array_equal(bits(ref["edges/floats"]), bits(want.astype(np.float32) / np.float32(255)))


EDGE_ROUNDINGS = 1 + 2 + 1          # e / 255; x - min and max - min; the quotient


def edge_bound_fraction(got, e):
    """|got - oracle| over EDGE_ROUNDINGS u |oracle|, worst over the image (an exact zero is exact on both sides)."""
    want = TO.normalised_edges(e)
    err = np.abs(got.astype(np.float64) - want)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(EDGE_ROUNDINGS * U * np.abs(want), 1e-300))))


@pytest.mark.parametrize("name", ("levels", "1x7", "2x5", "3x3", "floats"))
def test_normalised_edge_map_against_the_oracle(ref, name):
    img = ref["imgf/floats"] if name == "floats" else ref[f"img/{name}"]
    e = TO.edge_bytes_fast(img)
    assert e.max() > e.min()
    got = ops.find_edges(torch.from_numpy(img))
    assert got.dtype == torch.float32 and tuple(got.shape) == img.shape[1:]
    assert float(got.min()) == 0.0 and float(got.max()) == 1.0
    # the reference's own sequence on its own get_edges output, bit for bit
    x = torch.from_numpy(ref[f"edges/{name}"])
    assert torch.equal(got, (x - torch.min(x)) / (torch.max(x) - torch.min(x)))
    worst = edge_bound_fraction(got.numpy(), e)
    print(f"normalised edge map {name}: worst fraction of the {EDGE_ROUNDINGS} u bound {worst:.3f}")
    assert worst <= 1.0


def test_constant_image_gives_nan_and_uint8_equals_float(ref):
    # 0 / 0 where the EDGE image is constant: a black image of any size, a constant image without an interior pixel.  (A constant image
    # that is not black and has an interior is no such case under PIL's filter: its copied border is the grey value, its interior 0.)
    assert bool(torch.isnan(ops.find_edges(torch.zeros((3, 4, 6), dtype=torch.uint8))).all())
    assert bool(torch.isnan(ops.find_edges(torch.zeros((3, 4, 6)))).all())
    assert bool(torch.isnan(ops.find_edges(torch.full((3, 2, 5), 77, dtype=torch.uint8))).all())
    framed = ops.find_edges(torch.full((3, 4, 6), 77, dtype=torch.uint8))
    assert bool((framed[1:-1, 1:-1] == 0).all()) and float(framed.sum()) == 16.0
    assert bool(torch.isnan(ops.find_edges(torch.from_numpy(ref["img/1x1"]))).all())          # one pixel: max == min
    for name in IMAGES[:1] + IMAGES[2:]:
        img = torch.from_numpy(ref[f"img/{name}"])
        assert torch.equal(ops.find_edges(img), ops.find_edges(img.float() / 255.)), name
    for b in range(256):          # the / 255, * 255 round trip of the reference's uint8 branch is the identity on all 256 values
        assert int((torch.tensor(float(b)) / 255. * 255.).to(torch.uint8)) == b


def test_edge_maps_runs_find_edges_once_per_image(ref):
    train_set = [(None, ("name", torch.from_numpy(ref[f"img/{n}"]), None), None) for n in ("levels", "3x3")]
    maps = taming.edge_maps(train_set)
    assert len(maps) == 2 and all(torch.equal(m, ops.find_edges(t[1][1])) for m, t in zip(maps, train_set))
    maps = taming.edge_maps([(None, ("name", torch.from_numpy(ref["img/levels"]).float() / 255., None), None)], on_cpu=True)
    assert torch.equal(maps[0], ops.find_edges(torch.from_numpy(ref["img/levels"])))


def test_refusals():
    f = torch.ones(4)
    with pytest.raises(TypeError):
        ops.positive_medians(f)
    with pytest.raises(ValueError):
        ops.positive_medians([f] * 17)
    with pytest.raises(ValueError):
        ops.positive_medians([f, torch.ones(5)])
    with pytest.raises(NotImplementedError):
        ops.positive_medians([f.double()])
    with pytest.raises(NotImplementedError):
        ops.positive_medians([f.half()])
    c, m = ops.positive_medians([f])
    with pytest.raises(ValueError):
        ops.taming_score_accumulate_(torch.zeros(4), [f], [1.0, 2.0], c, m, torch.tensor(1.0), torch.ones(4, dtype=torch.bool), n_first=1)
    with pytest.raises(ValueError):
        ops.taming_score_accumulate_(torch.zeros(4), [f], [1.0], c, m, torch.tensor(1.0), torch.ones(4, dtype=torch.bool), n_first=2)
    with pytest.raises(NotImplementedError):
        ops.taming_score_accumulate_(torch.zeros(4), [f], [1.0], c, m, torch.tensor(1.0), torch.ones(4), n_first=1)
    with pytest.raises(ValueError):
        ops.find_edges(torch.zeros(4, 5, 5))
    with pytest.raises(NotImplementedError):
        ops.find_edges(torch.zeros(3, 5, 5, dtype=torch.float64))


def test_configuration_and_the_stand_alone_refusal():
    cfg = taming.HipTaming3DGSDensityController()
    assert cfg.budget == 20 and cfg.mode == "multiplier" and cfg.n_sample_cameras == 10 and cfg.cull_opacity_until == 27
    assert cfg.densification_interval == 500 and cfg.edges_on_cpu is False
    assert dataclasses.asdict(cfg.score_coeffs) == dict(
        view_importance=50, edge_importance=50, mse_importance=50, grad_importance=25, dist_importance=50, opac_importance=100,
        dept_importance=5, loss_importance=10, radii_importance=10, scale_importance=25, count_importance=0.1, blend_importance=50)
    assert cfg.score_coeffs is not taming.HipTaming3DGSDensityController().score_coeffs
    if not taming.INSIDE_REFERENCE:
        with pytest.raises(RuntimeError, match="VanillaDensityControllerImpl"):
            cfg.instantiate()


def test_header_section_is_additive():
    from gspl_amd import _lib as L
    text = open(L.HEADER_PATH).read()
    section = text[text.index("27. The scoring arithmetic of the Taming-3DGS"):]
    assert "PURELY ADDITIVE" in section and "no new struct" in section and L.ABI_VERSION == 39
    for name in ("gspl_positive_medians", "gspl_positive_medians_workspace_bytes", "gspl_taming_score_accumulate", "gspl_find_edges",
                 "gspl_find_edges_partials"):
        assert name in L.exported_symbols()
    assert L.GSPL_TAMING_MAX_ROWS == 16


def test_score_needs_a_renderer_with_projections():
    class Renderer:
        def training_forward(self, *a, **k):
            return {"render": torch.zeros(3, 2, 2), "visibility_filter": torch.ones(3, dtype=torch.bool)}

    class Model:
        n_gaussians = 3

        def get_scales(self):
            return torch.ones(3, 3)
    cams = [(object(), ("n", torch.zeros(3, 2, 2), None), None)]
    with pytest.raises(RuntimeError, match="opacities"):
        taming.compute_gaussian_score(Model(), Renderer(), 0, torch.zeros(3), cams, [torch.zeros(2, 2)], torch.zeros(3),
                                      taming.ScoreCoefficients(), 0.2)

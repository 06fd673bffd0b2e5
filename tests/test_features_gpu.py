"""Wide-feature compositing on the GPU (csrc/features.hip, `ops.rasterize_features`, the Feature-3DGS and SegAnyGS plugins).

Bounds are the project's own (tests/test_hip_parity.py::test_composite_fwd_bwd_vs_oracle): pixels the fp64 oracle does not flag as
fragile within 1e-5, every pixel within 1e-3, every gradient element within 1e-4 of |ref| + rms; and BIT equality with the narrow
compositing kernels, which follows from the shared sigma / alpha code and the list-order fmaf chain.

Scenes as test_hip_parity._composite_case builds them.  Checked with the oracle alone: 3000 splats at 97x65 (scale x3) leave every
pixel firm for tiles 8 / 16 / 32 (longest list 134 / 272 / 483); 6000 splats at 130x70 (scale x12, tile 16) saturate the image, walk
lists of up to 2053 entries and leave 0.9991 firm; 40 splats at 17x9 are all firm."""
import functools

import numpy as np
import pytest
import torch

import gspl_amd  # noqa: F401
from gspl_amd import _lib as L
from gspl_amd import ops
from oracle import gsplat_oracle as O

import feature_oracle as FO
from hip_helpers import assert_close_scaled, hip_composite_fwd

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HWC, CHW = L.GSPL_LAYOUT_HWC, L.GSPL_LAYOUT_CHW
SMALL, LONG, TINY = (3000, 97, 65, False), (6000, 130, 70, True), (40, 17, 9, True)


@functools.lru_cache(maxsize=None)
def _geometry(n, W, H, big, tile, mode):
    means, scales, quats, opac, _ = O.synthetic_scene(n, seed=11)
    cam = O.synthetic_camera(W, H, 260.0)
    res = O.project_gaussians(means, scales * (12.0 if big else 3.0), 1.0, quats, cam["world_to_camera"], cam["fx"], cam["fy"],
                              cam["cx"], cam["cy"], H, W)
    xys, depths, radii, conics, comp = res[0], res[1], res[2], res[3], res[4]
    op = (opac.reshape(-1) * comp).float()
    op[:min(20, n)] = 1.0                          # exercise the clamp
    if mode == O.MODE_INRIA:
        xys = xys - 0.5
    _, _, flat, offs = O.isect_tiles(mode, xys, radii, depths, W, H, block=tile)
    return xys.float(), conics.float(), op, torch.as_tensor(flat), torch.as_tensor(offs)


@functools.lru_cache(maxsize=None)
def _features(n, D):
    g = torch.Generator().manual_seed(11 + D)
    return torch.rand(n, D, generator=g), torch.rand(D, generator=g)


@functools.lru_cache(maxsize=None)
def _oracle_fwd(scene, tile, mode, D):
    """(out, alpha, last, fragile) of the fp64 oracle: computed once per case, shared, never modified."""
    n, W, H, big = scene
    xys, conics, op, flat, offs = _geometry(n, W, H, big, tile, mode)
    feats, bg = _features(n, D)
    return FO.feature_fwd(mode, xys, conics, feats, op, bg, W, H, offs, flat, tile=tile)


def _case(scene, tile, mode, D):
    n, W, H, big = scene
    xys, conics, op, flat, offs = _geometry(n, W, H, big, tile, mode)
    feats, bg = _features(n, D)
    c = lambda a: a.contiguous().to(DEV)
    return dict(n=n, W=W, H=H, tile=tile, mode=mode, D=D, cpu=(xys, conics, feats, op, bg, flat, offs),
                xys=c(xys), conics=c(conics), feats=c(feats), op=c(op), bg=c(bg), flat=c(flat), offs=c(offs))


def _new(shape, dtype=torch.float32, fill=None):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    if fill is not None:
        t.view(torch.uint8).fill_(fill)
    return t


def feature_fwd(k, layout=HWC, n_isects=None, offs=None, flat=None, fill=None, bufs=None):
    """gspl_feature_fwd through the C-ABI -> (out, alphas, final_Ts, last_ids)."""
    W, H, D, tile = k["W"], k["H"], k["D"], k["tile"]
    out, alphas, final_T, last = bufs or (_new((H, W, D) if layout == HWC else (D, H, W), fill=fill), _new((H, W), fill=fill),
                                          _new((H, W), fill=fill), _new((H, W), torch.int32, fill=fill))
    flat = k["flat"] if flat is None else flat
    n = flat.shape[0] if n_isects is None else n_isects
    rc = L.lib().gspl_feature_fwd(k["n"], n, D, k["mode"], layout, L.ptr(k["xys"]), L.ptr(k["conics"]), L.ptr(k["feats"]), L.ptr(k["op"]),
                                  L.ptr(k["bg"]), W, H, tile, (W + tile - 1) // tile, (H + tile - 1) // tile,
                                  L.ptr(k["offs"] if offs is None else offs), L.ptr(flat) if n else None,
                                  L.ptr(out), L.ptr(alphas), L.ptr(final_T), L.ptr(last), L.stream())
    L.check(rc, "gspl_feature_fwd")
    return out, alphas, final_T, last


def feature_bwd(k, last, v_out, layout=HWC, n_isects=None, offs=None, flat=None, v_features=None):
    W, H, D, tile = k["W"], k["H"], k["D"], k["tile"]
    v_features = torch.zeros((k["n"], D), device=DEV) if v_features is None else v_features
    flat = k["flat"] if flat is None else flat
    n = flat.shape[0] if n_isects is None else n_isects
    rc = L.lib().gspl_feature_bwd(k["n"], n, D, k["mode"], layout, L.ptr(k["xys"]), L.ptr(k["conics"]), L.ptr(k["op"]),
                                  W, H, tile, (W + tile - 1) // tile, (H + tile - 1) // tile,
                                  L.ptr(k["offs"] if offs is None else offs), L.ptr(flat), L.ptr(last), L.ptr(v_out), L.ptr(v_features), L.stream())
    L.check(rc, "gspl_feature_bwd")
    return v_features


def assert_same_up_to_summation_order(a, b, sum_abs, name, rel=1e-6):
    """Two runs of the atomic backward add the same per-block partial sums in different orders.  Reordering a sum of n fp32 terms moves
    it by at most (n - 1) 2^-24 sum|terms|, so the two results are compared RELATIVE TO THE SUM OF THE ABSOLUTE TERMS — `sum_abs`, the
    same backward run on |v_out| (the weights alpha T are non-negative) — not to the sum itself, which random signs cancel: 1e-6 of it
    allows for the 16 partial sums of a splat that covers sixteen 8x8 blocks."""
    a, b, sum_abs = (t.detach().double().cpu() for t in (a, b, sum_abs))
    assert float(sum_abs.max()) > 0 and bool((sum_abs >= 0).all())
    ratio = (a - b).abs() / (sum_abs + 1e-30)
    print(f"{name}: worst |a - b| / sum|terms| = {float(ratio.max()):.3e}")
    assert bool(((a - b).abs() <= rel * sum_abs).all()), f"{name}: worst {float(ratio.max()):.3e} of the sum of absolute terms"


def _hwc(img, layout):
    return img if layout == HWC else img.permute(1, 2, 0)


FWD_CASES = [(SMALL, 16, D, mode, layout) for D in (32, 40, 13, 128) for mode in (O.MODE_GSPLAT, O.MODE_INRIA) for layout in (HWC, CHW)] \
    + [(SMALL, tile, 40, O.MODE_GSPLAT, layout) for tile in (8, 32) for layout in (HWC, CHW)]
_fwd_id = lambda c: f"{c[0][1]}x{c[0][2]}-t{c[1]}-D{c[2]}-{'gsplat' if c[3] == O.MODE_GSPLAT else 'inria'}-{'hwc' if c[4] == HWC else 'chw'}"


# ---- 1. forward against the existing path: bit equality --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FWD_CASES, ids=_fwd_id)
def test_forward_is_bit_equal_to_the_narrow_kernels(case):
    scene, tile, D, mode, layout = case
    k = _case(scene, tile, mode, D)
    out, alphas, final_T, last = feature_fwd(k, layout)
    # the channel adapter over the narrow kernels (groups of 8), same lists
    ref, ref_alpha = ops._composite(k["xys"], k["conics"], k["feats"], k["op"], k["bg"], k["W"], k["H"], tile, k["offs"], k["flat"],
                                    False, mode, layout)
    assert torch.equal(out, ref) and torch.equal(alphas, ref_alpha)
    o8, a8, T8, l8 = hip_composite_fwd(mode, k["xys"], k["conics"], k["feats"][:, :8].contiguous(), k["op"], k["bg"][:8].contiguous(),
                                       k["W"], k["H"], k["offs"], k["flat"], tile=tile)
    assert torch.equal(final_T, T8) and torch.equal(last, l8) and torch.equal(alphas, a8)
    assert torch.equal(_hwc(out, layout)[..., :8], o8)
    if mode == O.MODE_GSPLAT:
        n = k["n"]
        dummy = torch.zeros(n, device=DEV)
        args = (k["xys"], dummy, dummy.int(), k["conics"], dummy.int(), k["feats"], k["op"][:, None], k["H"], k["W"], tile)
        kw = dict(background=k["bg"], return_alpha=True, isects=(k["flat"], k["offs"]), channels_first=layout == CHW)
        got, got_alpha = ops.rasterize_features(*args, **kw)
        want, want_alpha = ops.rasterize_gaussians(*args, **kw)
        assert torch.equal(got, want) and torch.equal(got_alpha, want_alpha) and torch.equal(got, out)


# ---- 2. forward against fp64 -----------------------------------------------------------------------------------------------------------
def _check_forward(k, scene, layout):
    out_ref, alpha_ref, last_ref, frag = _oracle_fwd(scene, k["tile"], k["mode"], k["D"])
    ok = frag == 0
    assert ok.mean() > 0.995
    out, alphas, final_T, last = feature_fwd(k, layout)
    diff = np.abs(_hwc(out, layout).cpu().numpy() - out_ref)
    print(f"forward: firm pixels {ok.mean():.4f}, worst firm {diff[ok].max():.3e}, worst {diff.max():.3e}")
    assert diff[ok].max() <= 1e-5
    assert np.abs(alphas.cpu().numpy() - alpha_ref)[ok].max() <= 1e-5
    assert np.abs(final_T.cpu().numpy() - (1.0 - alpha_ref))[ok].max() <= 1e-5
    assert np.array_equal(last.cpu().numpy()[ok], last_ref[ok])
    assert diff.max() <= 1e-3
    return frag, final_T, last


@pytest.mark.parametrize("case", FWD_CASES + [(LONG, 16, 40, O.MODE_GSPLAT, HWC), (LONG, 16, 40, O.MODE_INRIA, CHW)], ids=_fwd_id)
def test_forward_against_fp64(case):
    scene, tile, D, mode, layout = case
    _check_forward(_case(scene, tile, mode, D), scene, layout)


# ---- 3. backward against fp64 ----------------------------------------------------------------------------------------------------------
def _check_backward(k, scene, layout, through_autograd):
    """The direct C-ABI gradient against the oracle's v_colors (which differentiates the GPU's own alphas / last_ids); fragile pixels
    carry no loss."""
    W, H, D, tile, mode = k["W"], k["H"], k["D"], k["tile"], k["mode"]
    xys, conics, feats, op, bg, flat, offs = k["cpu"]
    frag = _oracle_fwd(scene, tile, mode, D)[3]
    assert (frag == 0).mean() > 0.995
    out, alphas, final_T, last = feature_fwd(k, layout)
    v_out = torch.randn(H, W, D, generator=torch.Generator().manual_seed(4))
    v_out[torch.from_numpy(frag != 0)] = 0.0
    v_dev = (v_out if layout == HWC else v_out.permute(2, 0, 1)).contiguous().to(DEV)
    got = feature_bwd(k, last, v_dev, layout)
    ref = FO.feature_bwd(mode, xys, conics, feats, op, bg, W, H, offs, flat, 1.0 - final_T.cpu().double().numpy(), last.cpu().numpy(),
                         v_out.double().numpy(), fragile_px=frag, tile=tile)
    assert float(np.abs(ref).max()) > 0
    assert_close_scaled(got.cpu().numpy(), ref, 1e-4, f"v_features D={D} tile={tile} mode={mode}", frac_ok=1.0)
    if through_autograd:
        f, b = k["feats"].clone().requires_grad_(True), k["bg"].clone().requires_grad_(True)
        dummy = torch.zeros(k["n"], device=DEV)
        img = ops.rasterize_features(k["xys"], dummy, dummy.int(), k["conics"], dummy.int(), f, k["op"][:, None], H, W, tile, background=b,
                                     isects=(k["flat"], k["offs"]), channels_first=layout == CHW)
        assert torch.equal(img, out)
        (img * v_dev).sum().backward()
        assert_close_scaled(f.grad.cpu().numpy(), got.cpu().numpy(), 1e-4, "features.grad against the direct call", frac_ok=1.0)
        want_bg = (v_out.double() * final_T.cpu().double()[..., None]).sum(dim=(0, 1))
        assert float(((b.grad.cpu().double() - want_bg).abs() / (want_bg.abs() + want_bg.abs().mean())).max()) <= 1e-5
        return img, f, v_dev
    return None


BWD_CASES = [(SMALL, tile, D, O.MODE_GSPLAT, CHW if tile == 16 else HWC) for D in (32, 40, 13, 128) for tile in (8, 16, 32)] \
    + [(SMALL, 16, 40, O.MODE_INRIA, HWC), (SMALL, 16, 32, O.MODE_INRIA, CHW), (SMALL, 16, 32, O.MODE_GSPLAT, HWC),
       (LONG, 16, 40, O.MODE_GSPLAT, HWC), (LONG, 16, 40, O.MODE_GSPLAT, CHW)]


@pytest.mark.parametrize("case", BWD_CASES, ids=_fwd_id)
def test_backward_against_fp64(case):
    scene, tile, D, mode, layout = case
    _check_backward(_case(scene, tile, mode, D), scene, layout, through_autograd=mode == O.MODE_GSPLAT)


# ---- 4. 256 channels -------------------------------------------------------------------------------------------------------------------
def test_256_channels_forward_and_backward():
    k = _case(SMALL, 16, O.MODE_GSPLAT, 256)
    _check_forward(k, SMALL, CHW)
    _check_backward(k, SMALL, CHW, through_autograd=True)


# ---- 5. edges --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [HWC, CHW])
def test_no_splats_and_empty_lists_give_the_background(layout):
    W, H, D = 37, 21, 40
    bg = torch.rand(D, device=DEV)
    want = bg.expand(H, W, D) if layout == HWC else bg[:, None, None].expand(D, H, W)
    offs = torch.zeros(((W + 15) // 16) * ((H + 15) // 16), dtype=torch.int32, device=DEV)
    empty = dict(n=0, W=W, H=H, tile=16, mode=O.MODE_GSPLAT, D=D, xys=None, conics=None, feats=None, op=None, bg=bg,
                 flat=torch.zeros(0, dtype=torch.int32, device=DEV), offs=offs)
    some = _case(TINY, 16, O.MODE_GSPLAT, D)
    listless = dict(some, W=W, H=H, bg=bg, flat=empty["flat"], offs=offs)
    for k in (empty, listless):
        out, alphas, final_T, last = feature_fwd(k, layout, fill=0xFF)
        assert torch.equal(out, want) and not bool(alphas.any()) and bool((final_T == 1).all()) and not bool(last.any())
        v = feature_bwd(k, last, torch.ones_like(out), layout)
        assert not bool(v.any())
    # the op: N == 0
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)
    f = z(0, D).requires_grad_(True)
    b = bg.clone().requires_grad_(True)
    img, alpha = ops.rasterize_features(z(0, 2), z(0), z(0, dt=torch.int32), z(0, 3), z(0, dt=torch.int32), f, z(0, 1), H, W, 16,
                                        background=b, return_alpha=True, channels_first=layout == CHW)
    assert torch.equal(img, want) and not bool(alpha.any())
    img.sum().backward()
    assert f.grad.shape == (0, D) and torch.allclose(b.grad, torch.full((D,), float(H * W), device=DEV))


@pytest.mark.parametrize("D,layout", [(40, HWC), (40, CHW), (1, HWC), (1, CHW)])
def test_tiny_image_and_one_channel(D, layout):
    for scene in (TINY, SMALL) if D == 1 else (TINY,):
        k = _case(scene, 16, O.MODE_GSPLAT, D)
        _check_forward(k, scene, layout)
        _check_backward(k, scene, layout, through_autograd=True)


def test_device_side_list_length():
    """n_isects < 0: `offsets` carries one more entry, the list length; the list buffer is longer than the list."""
    k = _case(SMALL, 16, O.MODE_GSPLAT, 40)
    n = k["flat"].shape[0]
    offs_ext = torch.cat([k["offs"], torch.tensor([n], dtype=torch.int32, device=DEV)])
    flat_cap = torch.cat([k["flat"], torch.full((1000,), k["n"] - 1, dtype=torch.int32, device=DEV)])      # (never to be read)
    want = feature_fwd(k, CHW)
    got = feature_fwd(k, CHW, n_isects=-1, offs=offs_ext, flat=flat_cap)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    v_out = torch.randn(want[0].shape, generator=torch.Generator().manual_seed(2)).to(DEV)
    a = feature_bwd(k, want[3], v_out, CHW)
    b = feature_bwd(k, want[3], v_out, CHW, n_isects=-1, offs=offs_ext, flat=flat_cap)
    assert_same_up_to_summation_order(b, a, feature_bwd(k, want[3], v_out.abs(), CHW), "device-side list length")


def test_lists_binned_by_the_op_and_a_second_backward():
    """The op's own binning (lists whose length stays on the device) gives rasterize_gaussians' image; backward twice through
    retain_graph gives the same gradient (atomics: to 1e-6 of the sum of the absolute terms)."""
    n, W, H = 3000, 97, 65
    means, scales, quats, opac, _ = [t.to(DEV) for t in O.synthetic_scene(n, seed=11)]
    cam = O.synthetic_camera(W, H, 260.0)
    vm = cam["world_to_camera"].T.contiguous().float().to(DEV)
    xys, depths, radii, conics, comp, tiles, _ = ops.project_gaussians(means, scales * 3, 1.0, quats, vm, cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                                                                       H, W, 16, return_cov3d=False)
    feats, bg = [t.to(DEV) for t in _features(n, 40)]
    f = feats.clone().requires_grad_(True)
    op = opac * comp[:, None]
    for _ in range(2):      # the second frame has a capacity guess: LazyLists
        got = ops.rasterize_features(xys, depths, radii, conics, tiles, f, op, H, W, 16, background=bg)
        want = ops.rasterize_gaussians(xys, depths, radii, conics, tiles, feats, op, H, W, 16, background=bg)
        assert torch.equal(got, want)
    w = torch.randn(H, W, 40, generator=torch.Generator().manual_seed(3)).to(DEV)
    loss = (got * w).sum()
    loss.backward(retain_graph=True)
    g1 = f.grad.clone()
    f.grad = None
    loss.backward(retain_graph=True)
    g2 = f.grad.clone()
    f.grad = None
    (got * w.abs()).sum().backward()
    assert float(g1.abs().max()) > 0
    assert_same_up_to_summation_order(g2, g1, f.grad, "second backward")


# ---- 6. no write outside the buffers ---------------------------------------------------------------------------------------------------
GUARD = 4096


def _carved(nbytes, fill):
    outer = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    inner = outer[GUARD:GUARD + nbytes]
    inner.fill_(fill)
    return outer, inner


@pytest.mark.parametrize("D", [13, 40])
@pytest.mark.parametrize("layout", [HWC, CHW], ids=["hwc", "chw"])
def test_no_write_outside_the_buffers(D, layout):
    k = _case(SMALL, 16, O.MODE_GSPLAT, D)
    W, H, n = k["W"], k["H"], k["n"]
    P = W * H
    v_out = torch.randn((H, W, D) if layout == HWC else (D, H, W), generator=torch.Generator().manual_seed(6)).to(DEV)
    results = []
    for fill in (0xFF, 0x00):
        sizes = {"out": 4 * P * D, "alphas": 4 * P, "final_T": 4 * P, "last": 4 * P, "v_features": 4 * n * D}
        bufs = {name: _carved(nb, 0x00 if name == "v_features" else fill) for name, nb in sizes.items()}
        f32 = lambda name, shape: bufs[name][1].view(torch.float32).view(shape)
        outs = (f32("out", v_out.shape), f32("alphas", (H, W)), f32("final_T", (H, W)), bufs["last"][1].view(torch.int32).view(H, W))
        feature_fwd(k, layout, bufs=outs)
        feature_bwd(k, outs[3], v_out, layout, v_features=f32("v_features", (n, D)))
        torch.cuda.synchronize()
        for name, nb in sizes.items():
            outer = bufs[name][0]
            assert bool((outer[:GUARD] == 0xA5).all()) and bool((outer[GUARD + nb:] == 0xA5).all()), f"a write outside {name}"
        results.append([t.clone() for t in outs] + [f32("v_features", (n, D)).clone()])
    for a, b in zip(results[0][:4], results[1][:4]):
        assert torch.equal(a, b)          # every element written: nothing of the pre-fill shows
    assert bool(torch.isfinite(results[0][0]).all()) and float(results[0][4].abs().max()) > 0


# ---- 7. fallback and refusals ----------------------------------------------------------------------------------------------------------
def _op_args(k):
    dummy = torch.zeros(k["n"], device=DEV)
    return (k["xys"], dummy, dummy.int(), k["conics"], dummy.int()), dict(background=k["bg"], return_alpha=True, isects=(k["flat"], k["offs"]))


def test_geometry_gradients_fall_back_to_the_general_path():
    k = _case(SMALL, 16, O.MODE_GSPLAT, 40)
    w = torch.randn(k["H"], k["W"], 40, generator=torch.Generator().manual_seed(8)).to(DEV)
    runs = []
    for fn in (ops.rasterize_features, ops.rasterize_gaussians):
        (xys, *rest), kw = _op_args(k)
        xys, f = xys.clone().requires_grad_(True), k["feats"].clone().requires_grad_(True)
        img, alpha = fn(xys, *rest, f, k["op"][:, None], k["H"], k["W"], 16, **kw)
        (img * w).sum().backward()
        runs.append((img, alpha, xys.grad, f.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert float(runs[0][2].abs().max()) > 0
    for a, b, name in zip(runs[0][2:], runs[1][2:], ("means2d.grad", "features.grad")):      # (atomics: the order of the additions differs)
        assert_close_scaled(a.cpu().numpy(), b.cpu().numpy(), 1e-5, name, frac_ok=1.0)


def test_deterministic_mode_is_bit_reproducible():
    k = _case(LONG, 16, O.MODE_GSPLAT, 40)
    w = torch.randn(k["H"], k["W"], 40, generator=torch.Generator().manual_seed(9)).to(DEV)
    old = L.lib().gspl_set_deterministic(1)
    try:
        grads = []
        for _ in range(2):
            args, kw = _op_args(k)
            f = k["feats"].clone().requires_grad_(True)
            img, _ = ops.rasterize_features(*args, f, k["op"][:, None], k["H"], k["W"], 16, **kw)
            (img * w).sum().backward()
            grads.append(f.grad)
        assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0
    finally:
        L.lib().gspl_set_deterministic(old)


def test_bad_arguments_are_refused():
    k = _case(TINY, 16, O.MODE_GSPLAT, 40)
    sentinel = lambda: feature_fwd(k, HWC, fill=0xFF)      # placeholder shapes
    out, alphas, final_T, last = [t.fill_(7) for t in sentinel()]
    v_out, v_f = torch.ones_like(out), torch.zeros(k["n"], 40, device=DEV)

    def refused(code, match, **bad):
        kk = dict(k, **{n: v for n, v in bad.items() if n in k})
        layout = bad.get("layout", HWC)
        with pytest.raises(RuntimeError, match=match) as e:
            if bad.get("which", "fwd") == "fwd":
                feature_fwd(kk, layout, bufs=bad.get("bufs", (out, alphas, final_T, last)))
            else:
                feature_bwd(kk, bad.get("last", last), bad.get("v_out", v_out), layout, v_features=v_f)
        assert f"status {code}" in str(e.value)

    for which in ("fwd", "bwd"):
        refused(L.GSPL_ERR_INVALID_ARG, "bad argument", which=which, D=0)
        refused(L.GSPL_ERR_INVALID_ARG, "bad argument", which=which, mode=7)
        refused(L.GSPL_ERR_INVALID_ARG, "bad argument", which=which, layout=5)
        refused(L.GSPL_ERR_UNSUPPORTED, "tile_size", which=which, tile=12)
        refused(L.GSPL_ERR_INVALID_ARG, "NULL", which=which, conics=None)
    refused(L.GSPL_ERR_INVALID_ARG, "NULL", which="fwd", feats=None)
    refused(L.GSPL_ERR_INVALID_ARG, "NULL", which="fwd", bufs=(out, None, final_T, last))
    refused(L.GSPL_ERR_INVALID_ARG, "NULL", which="bwd", v_out=None)
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((last == 7).all()) and not bool(v_f.any())      # nothing was launched


def test_no_host_synchronisation():
    k = _case(SMALL, 16, O.MODE_GSPLAT, 40)
    args, kw = _op_args(k)
    f, b = k["feats"].clone().requires_grad_(True), k["bg"].clone().requires_grad_(True)
    kw["background"] = b
    w = torch.randn(40, k["H"], k["W"], generator=torch.Generator().manual_seed(5)).to(DEV)
    op = k["op"][:, None].contiguous()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        img, alpha = ops.rasterize_features(*args, f, op, k["H"], k["W"], 16, channels_first=True, **kw)
        (img * w).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(f.grad).all()) and float(f.grad.abs().max()) > 0 and bool(torch.isfinite(b.grad).all())


# ---- 8. the plugins --------------------------------------------------------------------------------------------------------------------
class _Module:
    def __init__(self, model):
        self.gaussian_model, self.device = model, DEV


def _plugin_scene(n=3000, W=97, H=65):
    from fakes import FakeCamera, FakePropertyModel
    means, scales, quats, opac, shs = O.synthetic_scene(n, seed=11)
    model = FakePropertyModel(*[t.to(DEV) for t in (means, scales * 3, quats, opac, shs)])
    cam = O.synthetic_camera(W, H, 260.0)
    return model, cam, FakeCamera(cam, DEV)


@pytest.mark.parametrize("speedup,dims", [(False, 32), (True, 64)])
def test_feature_3dgs_plugin(speedup, dims):
    from gspl_amd.renderers import HipFeature3DGSRenderer, HipGSplatRenderer
    model, _, cam = _plugin_scene()
    n, W, H = model.n_gaussians, 97, 65
    torch.manual_seed(0)
    r = HipFeature3DGSRenderer(speedup=speedup, n_feature_dims=dims)
    r.setup("fit", lightning_module=_Module(model))
    raw_dims = dims // 2 if speedup else dims
    assert r.n_actual_feature_dims == raw_dims and r.features.shape == (n, raw_dims) and not bool(r.features.any())
    optimizer, scheduler = r.training_setup(None)
    assert scheduler is None and [g["name"] for g in optimizer.param_groups] == ["features", "feature_decoder"]
    assert [g["lr"] for g in optimizer.param_groups] == [0.001, 0.0001]
    with torch.no_grad():
        r.features.copy_(torch.randn(n, raw_dims, generator=torch.Generator().manual_seed(1)))
    bg = torch.tensor([0.1, 0.3, 0.6], device=DEV)
    out = r(cam, model, bg, render_types=["rgb", "features", "features_pca_3d", "edited"])
    assert set(out) == {"render", "raw_features", "features", "features_pca_3d", "edited"}
    assert out["render"].shape == out["features_pca_3d"].shape == out["edited"].shape == (3, H, W)
    assert out["raw_features"].shape == (raw_dims, H, W) and out["features"].shape == (dims, H, W)
    assert torch.equal(out["features"], r.feature_decoder(out["raw_features"]))
    assert torch.equal(out["edited"], out["render"]) and r.pca_projected_color.shape == (n, 3)
    r.edit_mask = (torch.arange(n, device=DEV) % 2 == 0).float()
    assert not torch.equal(r(cam, model, bg, render_types=["edited"])["edited"], out["render"])
    assert set(r.training_forward(0, None, cam, model, bg)) == {"raw_features", "features"}
    # the route of the parent commit: `rasterize_simplified` in batches of 32 channels
    with torch.no_grad():
        proj = HipGSplatRenderer.project(model.get_xyz, model.get_scaling, model.get_rotation, cam)
        opac = model.get_opacity * proj[4][:, None]
        zero = torch.zeros(32, device=DEV)
        batched = torch.cat([HipGSplatRenderer.rasterize_simplified(proj, cam, r.features[:, s:s + 32], zero, opac, anti_aliased=False)
                             for s in range(0, raw_dims, 32)])
    assert torch.equal(out["raw_features"].detach(), batched)
    # training: only the renderer's own parameters receive gradients, and they learn
    target = torch.randn(dims, H, W, generator=torch.Generator().manual_seed(2)).to(DEV) * 0.1 + 0.3
    losses = []
    for step in range(10):
        optimizer.zero_grad(set_to_none=True)
        loss = (r.training_forward(step, None, cam, model, bg)["features"] - target).abs().mean()
        loss.backward()
        if step == 0:
            assert r.features.grad is not None and float(r.features.grad.abs().max()) > 0
            assert all(p.grad is not None for p in r.feature_decoder.parameters())
            assert all(p.grad is None for p in model.properties.values())
        optimizer.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0]


@pytest.mark.parametrize("width", [-1, 48])
def test_contrastive_feature_plugin(width):
    from fakes import FakeCamera
    from gspl_amd.renderers import HipGSplatContrastiveFeatureRenderer, HipGSplatRenderer
    model, cam_dict, cam = _plugin_scene()
    for p in model.properties.values():
        p.requires_grad_(False)                  # SegAnyGS trains features over a frozen model
    n, W, H = model.n_gaussians, 97, 65
    w, h = (W, H) if width < 0 else (width, int(width * H / W))
    feats = torch.randn(n, 32, generator=torch.Generator().manual_seed(3)).to(DEV).requires_grad_(True)
    bg = torch.zeros(32, device=DEV)
    r = HipGSplatContrastiveFeatureRenderer(feature_map_width=width)
    out = r(cam, model, bg, semantic_features=feats)
    assert set(out) == {"render", "viewspace_points", "viewspace_points_grad_scale", "visibility_filter", "radii"}
    assert out["render"].shape == (32, h, w) and out["viewspace_points_grad_scale"] == 0.5 * max(h, w)
    # HipGSplatRenderer's projection and the existing rasterizer at the rescaled intrinsics
    scaled = dict(cam_dict, width=w, height=h, fx=cam_dict["fx"] * (w / W), fy=cam_dict["fy"] * (h / H), cx=cam_dict["cx"] * (w / W),
                  cy=cam_dict["cy"] * (h / H))
    ref_cam = FakeCamera(scaled, DEV)
    proj = HipGSplatRenderer.project(model.get_xyz, model.get_scaling, model.get_rotation, ref_cam)
    xys, depths, radii, conics, comp, tiles, _ = proj
    ref = ops.rasterize_gaussians(xys, depths, radii, conics, tiles, feats.detach(), model.get_opacity * comp[:, None], h, w, 16, background=bg)
    assert torch.equal(out["render"].detach(), ref.permute(2, 0, 1)) and torch.equal(out["radii"], radii)
    out["render"].square().sum().backward()
    assert float(feats.grad.abs().max()) > 0
    depth = r.depth_forward(cam, model)
    want = HipGSplatRenderer()(cam, model, torch.zeros(3, device=DEV), render_types=["acc_depth"])["acc_depth"]
    assert depth.shape == (1, H, W) and float(depth.max()) > 1
    # (HipGSplatRenderer normalises the rotations first, the contrastive renderer takes them as stored: unit quaternions up to rounding)
    assert torch.allclose(depth, want, rtol=1e-5, atol=1e-5)

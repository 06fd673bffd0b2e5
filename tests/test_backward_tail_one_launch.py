"""The backward tail of the fused Inria call in its one-launch form: the gradient arrays are cleared by extra workgroups at the front of
the compositing backward's grid (csrc/composite_bwd.hip, FILL; a launch of its own when the frame has no lists), and ONE per-splat
kernel behind it does the SH backward and the geometry backward of the rows that have a gradient (csrc/inria.hip, SHDEG >= 0).

The contract is the one of tests/test_sparse_backward_tail.py: for identical inputs, in the deterministic mode, every output of a step
through this path equals the dense path's (`ops.SPARSE_TAIL = False`) AS A VALUE (`torch.equal`: a zero may differ in sign, nothing
else may differ) — all parameter gradients, the screen-space gradient, the three densification buffers, the row flags (against `!= 0`
of the dense path's packed rows), and parameters and both moments after `FusedAdam.step()`.  No tolerance.

Shapes: a 40 x 24 image (3 x 2 tiles, the right column and the bottom row partial) and N in {1, 63, 257, 1031}: arrays of 1, 3, 4 and
6 floats per row whose lengths are no multiples of four (the fill's head / body / tail), one block of the per-splat kernel and several,
compaction across wave and block edges.  Which rows have a gradient is built into the scenes, and checked against the dense path:
a row is `live` (faint, in view), `dead` (behind the camera: radius 0) or `hidden` (in view behind a wall of opaque splats: radius > 0,
no gradient)."""
import pytest
import torch

from oracle import gsplat_oracle as O

pytestmark = pytest.mark.gpu

W, H, FX = 40, 24, 60.0
BG = torch.tensor([0.25, 0.5, 0.125])
NAMES = ("means", "scales", "rotations", "opacities", "shs_dc", "shs_rest")
LRS = (1.6e-4, 5e-3, 1e-3, 5e-2, 2.5e-3, 2.5e-3 / 20)
SIZES = (1, 63, 257, 1031)


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib, ops
    _lib.lib()
    return ops


@pytest.fixture(autouse=True)
def _deterministic_and_restored(hip):
    was_det, was_sparse, was_seg = hip.set_deterministic(True), hip.SPARSE_TAIL, hip.SEGMENTED_BACKWARD
    yield
    hip.set_deterministic(was_det)
    hip.SPARSE_TAIL, hip.SEGMENTED_BACKWARD, hip.KEEP_LAST_RASTER = was_sparse, was_seg, False


def _dev():
    return torch.device("cuda:0")


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def _pattern(n, kind):
    """Per row: 0 dead (behind the camera), 1 live, 2 hidden behind the wall, 3 a wall splat."""
    idx = torch.arange(n)
    if kind == "all":
        return torch.ones(n, dtype=torch.long)
    if kind == "culled":
        return torch.zeros(n, dtype=torch.long)
    if kind == "one_per_block":      # exactly one row of every 256-row block of the per-splat kernel (the last block: if it is that long)
        return (idx % 256 == (40 if n > 40 else 0)).long()
    if kind == "last_wave":          # the live rows of a block all in its last wave
        return (idx % 256 >= 192).long()
    if kind == "wall":               # eight opaque splats across the image in front; behind them two rows in three in view, one dead
        kinds = torch.where(idx % 3 == 2, 0, 2)
        kinds[:8] = 3
        return kinds
    raise ValueError(kind)


def _scene(n, K, kind, seed=3):
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    kinds = _pattern(n, kind)
    faint = int((kinds == 1).sum()) > 64      # many live rows: nearly transparent, so that none hides another
    means = u(n, 3) * torch.tensor([1.0, 0.6, 0.3])                    # in view: the image spans +-1.33 x +-0.8 at the origin's depth
    scales = 0.1 + 0.1 * torch.rand(n, 3, generator=g)                 # 1.5 - 3 pixels
    opac = (0.02 + 0.03 * torch.rand(n, 1, generator=g)) if faint else (0.4 + 0.2 * torch.rand(n, 1, generator=g))
    dead, hidden, wall = kinds == 0, kinds == 2, kinds == 3
    means[dead, 2] -= 6.0                                              # the camera stands at z = -4 and looks along +z
    means[hidden, 2] += 1.5
    means[wall] = u(int(wall.sum()), 3) * torch.tensor([0.05, 0.05, 0.2]) + torch.tensor([0.0, 0.0, -1.5])
    scales[wall] = 6.0                                                 # sigma 120 pixels: alpha 0.99 over the whole image, T < 1e-4 behind two
    opac[wall] = 0.99
    quats = torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=-1)
    shs = torch.randn(n, K, 3, generator=g) * 0.3
    return (means, scales, quats, opac, shs), kinds


def _camera():
    return O.synthetic_camera(W, H, FX)


def _settings(hip, cam, deg, accel=False):
    make = hip.AccelRasterizationSettings if accel else hip.GaussianRasterizationSettings
    return make(image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=BG.to(_dev()), scale_modifier=1.0,
                viewmatrix=cam["world_to_camera"].to(_dev()), projmatrix=cam["full_projection"].to(_dev()), sh_degree=deg,
                campos=cam["camera_center"].to(_dev()))


def _leaves(scene, raw, split):
    means, scales, quats, opac, shs = scene
    if raw:
        scales, opac, quats = torch.log(scales), torch.logit(opac), quats * 1.7
    ts = [means, scales, quats, opac] + ([shs[:, :1], shs[:, 1:]] if (split and shs.shape[1] > 1) else [shs])
    return [t.clone().contiguous().to(_dev()).requires_grad_(True) for t in ts]


def _weights(channels=3, seed=1):
    return torch.randn(channels, H, W, generator=torch.Generator().manual_seed(seed)).to(_dev())


def _poison_free_blocks(leaves):
    """Blocks of the gradient tensors' sizes (and of the row flags'), full of NaN, given back to the caching allocator: what the
    backward's `torch.empty` calls are handed next."""
    n = leaves[0].shape[0]
    blocks = [torch.full_like(t, float("nan")) for t in leaves for _ in range(3)]
    blocks += [torch.full((n, 3), float("nan"), device=_dev()) for _ in range(3)]
    blocks += [torch.full((n,), 0xFF, dtype=torch.uint8, device=_dev()) for _ in range(3)]
    torch.cuda.synchronize()
    del blocks


def _stats0(n):
    g = torch.Generator().manual_seed(9)
    return [torch.rand(n, generator=g).to(_dev()), torch.randint(0, 5, (n,), generator=g).float().to(_dev()), (torch.rand(n, generator=g) * 5).to(_dev())]


def _step(hip, scene, *, sparse, deg, raw=False, split=True, aa=False, invd=False, v_zero=False, stale=False, adam=True):
    """One forward + backward with the densification statistics taken along, then one FusedAdam step: every output as a dict."""
    from gspl_amd import optimizers
    from gspl_amd.density import request_stats_in_backward
    hip.SPARSE_TAIL, hip.KEEP_LAST_RASTER = sparse, True
    leaves = _leaves(scene, raw, split)
    n = leaves[0].shape[0]
    names = NAMES if len(leaves) == 6 else NAMES[:4] + ("shs",)
    stats = _stats0(n)
    m, s, q, o, *sh = leaves
    screen = torch.zeros_like(m, requires_grad=True)
    dc, rest = (sh[0], sh[1]) if len(sh) == 2 else (sh[0], None)
    inv = None
    if aa or invd:
        render, radii, inv = hip.rasterize_inria_accel(_settings(hip, _camera(), deg, accel=True), m, screen, o, shs=dc, scales=s, rotations=q, shs_rest=rest,
                                                       raw_parameters=raw, antialiasing=aa, inverse_depth=invd)
    else:
        render, radii = hip.GaussianRasterizer(_settings(hip, _camera(), deg))(means3D=m, means2D=screen, opacities=o, shs=dc, shs_rest=rest, scales=s,
                                                                              rotations=q, raw_parameters=raw)
    loss = (render * _weights()).sum() + (0 if inv is None else (inv * _weights(1, seed=2)).sum())
    if v_zero:
        loss = loss * 0.0
    request = request_stats_in_backward(radii, *stats)
    assert request is not None
    if stale:
        _poison_free_blocks(leaves)
    loss.backward()
    torch.cuda.synchronize()
    assert request.applied
    out = {name: t.grad.clone() for name, t in zip(names, leaves)}
    out["viewspace"] = screen.grad.clone()
    out.update(accum=stats[0], denom=stats[1], max_radii=stats[2], radii=radii, render=render.detach())
    last = hip.LAST_RASTER
    out["packed"] = last["packed_grads"].clone()
    out["grad_rows"] = None if last.get("grad_rows") is None else last["grad_rows"].clone()
    tag = getattr(leaves[0].grad.untyped_storage(), "_gspl_grad_rows", None)
    assert (tag is None) == (out["grad_rows"] is None)
    if adam:
        opt = optimizers.FusedAdam([{"params": [t], "lr": lr, "name": name} for t, lr, name in zip(leaves, LRS, names)], eps=1e-15)
        opt.step()
        torch.cuda.synchronize()
        for name, t in zip(names, leaves):
            st = opt.state[t]
            out["adam." + name], out["adam." + name + ".exp_avg"], out["adam." + name + ".exp_avg_sq"] = t.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    hip.KEEP_LAST_RASTER = False
    return out


def _nonzero_rows(out):
    n = out["means"].shape[0]
    nz = torch.zeros(n, dtype=torch.bool, device=_dev())
    for name, t in out.items():
        if name in NAMES or name in ("shs", "viewspace"):
            nz |= (t.reshape(n, -1) != 0).any(dim=1)
    return nz


def _assert_same(ref, got, what):
    assert ref["grad_rows"] is None and got["grad_rows"] is not None, f"{what}: the switch did not select the two paths"
    for name, r in ref.items():
        if name in ("grad_rows", "packed"):
            continue
        g = got[name]
        assert not torch.isnan(g.float()).any(), f"{what}: NaN in {name}"
        assert torch.equal(r, g), f"{what}: {name} differs in {int((r != g).sum())} elements (max |diff| {float((r.float() - g.float()).abs().max()):.3e})"
    flags = got["grad_rows"]
    assert flags.dtype == torch.uint8 and flags.shape == (ref["means"].shape[0],)
    expect = (ref["packed"] != 0).any(dim=1)      # where the dense path defines the flag: through its packed rows
    assert torch.equal(flags, expect.to(torch.uint8)), f"{what}: {int((flags != expect.to(torch.uint8)).sum())} row flags differ from `!= 0` of the dense path's packed rows"
    missed = _nonzero_rows(ref) & (flags == 0)
    assert not bool(missed.any()), f"{what}: {int(missed.sum())} rows with a non-zero gradient carry flag 0"


def _compare(hip, scene, what, **kw):
    stale = kw.pop("stale", False)
    ref = _step(hip, scene, sparse=False, **kw)
    got = _step(hip, scene, sparse=True, stale=stale, **kw)
    _assert_same(ref, got, what)
    return ref, got


# ---- which rows have a gradient ----------------------------------------------------------------------------------------------------------
# (N = 1 and 63 have no last wave, and no room behind a wall of eight)
@pytest.mark.parametrize("n,kind", [(n, kind) for kind in ("all", "one_per_block") for n in SIZES] + [(n, kind) for kind in ("last_wave", "wall") for n in (257, 1031)])
def test_row_patterns(hip, n, kind):
    scene, kinds = _scene(n, 16, kind)
    kinds = kinds.to(_dev())
    ref, got = _compare(hip, scene, f"N={n} {kind}", deg=3)
    live, visible = _nonzero_rows(ref), ref["radii"] > 0
    assert torch.equal(visible, kinds != 0), "the scene's dead rows are not the rows behind the camera"
    if kind != "wall":
        assert torch.equal(live, kinds == 1), f"the scene does not have the pattern it was built for: {int(live.sum())} rows with a gradient, {int((kinds == 1).sum())} meant"
    else:
        assert not bool(live[kinds == 2].any()) and bool(live[kinds == 3].any()) and int((kinds == 2).sum()) > 0, "the wall does not hide the rows behind it"
    # visible rows without a gradient still count for the densification statistics
    accum0, denom0, max0 = _stats0(n)
    assert torch.equal(got["denom"], denom0 + visible.float())
    assert torch.equal(got["max_radii"], torch.where(visible, torch.maximum(max0, got["radii"].float()), max0))
    assert torch.equal(got["accum"][~live], accum0[~live])


@pytest.mark.parametrize("n", SIZES)
def test_no_row_with_a_gradient(hip, n):
    """v_out = 0: the lists are there, every packed row is zero."""
    scene, _ = _scene(n, 16, "all")
    ref, got = _compare(hip, scene, f"N={n} v_out=0", deg=3, v_zero=True)
    assert not bool(_nonzero_rows(got).any()) and int(got["grad_rows"].sum()) == 0
    assert bool((got["radii"] > 0).all()) and torch.equal(got["denom"], _stats0(n)[1] + 1.0)


@pytest.mark.parametrize("n", SIZES)
def test_every_splat_culled(hip, n):
    """No list entry, no compositing launch for the fill to ride in: the gradients still come back zero out of poisoned memory."""
    scene, _ = _scene(n, 16, "culled")
    ref, got = _compare(hip, scene, f"N={n} culled", deg=3, stale=True)
    assert not bool((got["radii"] > 0).any()) and not bool(_nonzero_rows(got).any()) and int(got["grad_rows"].sum()) == 0
    for name in NAMES + ("viewspace",):
        assert not bool((got[name] != 0).any()), name


@pytest.mark.parametrize("n", [257, 1031])
@pytest.mark.parametrize("kind", ["one_per_block", "wall"])
def test_poisoned_allocator_blocks(hip, n, kind):
    scene, _ = _scene(n, 16, kind)
    _compare(hip, scene, f"stale blocks, N={n} {kind}", deg=3, stale=True)


# ---- the routes of the per-splat kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg,K,split,raw", [(0, 1, False, False), (0, 1, False, True), (0, 16, True, False), (0, 16, False, True), (1, 16, True, True), (1, 16, False, False), (2, 9, True, False),
                                             (3, 16, True, True), (3, 16, False, True), (3, 16, False, False)])
def test_sh_layouts_and_parameter_forms(hip, deg, K, split, raw):
    """n_coeffs above the active degree: the columns above it stay the fill's zeros.  Half the rows live, every third dead."""
    n = 257
    scene, kinds = _scene(n, K, "all")
    scene[0][torch.arange(n) % 3 == 2, 2] -= 6.0
    ref, got = _compare(hip, scene, f"degree={deg} K={K} split={split} raw={raw}", deg=deg, raw=raw, split=split)
    rest = got["shs_rest"] if "shs_rest" in got else got["shs"]
    rest = rest.reshape(n, -1)[:, (0 if "shs_rest" in got else 3):]
    active = 3 * ((deg + 1) ** 2 - 1)
    assert not bool((rest[:, active:] != 0).any()), "coefficient columns above the active degree were written"
    assert 0 < int(_nonzero_rows(ref).sum()) < n


@pytest.mark.parametrize("aa,invd", [(True, False), (False, True)])
@pytest.mark.parametrize("raw", [False, True])
def test_antialiasing_and_inverse_depth(hip, aa, invd, raw):
    scene, _ = _scene(1031, 16, "wall")
    ref, _got = _compare(hip, scene, f"antialias={aa} invdepth={invd} raw={raw}", deg=3, raw=raw, aa=aa, invd=invd)
    assert 0 < int(_nonzero_rows(ref).sum()) < 1031


def test_a_second_backward_with_another_n(hip):
    """One process, backwards of different sizes and kinds one after the other: no FillJob or flag of a call survives into the next."""
    order = [(1031, "all"), (63, "one_per_block"), (257, "culled"), (1031, "wall"), (1, "all"), (257, "last_wave")]
    scenes = [_scene(n, 16, kind)[0] for n, kind in order]
    refs = [_step(hip, sc, sparse=False, deg=3, adam=False) for sc in scenes]
    for (n, kind), sc, ref in zip(order, scenes, refs):
        _assert_same(ref, _step(hip, sc, sparse=True, deg=3, adam=False, stale=True), f"in sequence: N={n} {kind}")


# ---- the segmented compositing backward: two launches, the fill rides in the first ---------------------------------------------------------
def _close(a, b, name, rel=5e-5):
    a, b = a.double(), b.double()
    rms = float(b.pow(2).mean().sqrt()) + 1e-30
    ratio = (a - b).abs() / (b.abs() + rms)
    assert float(ratio.max()) <= rel, f"{name}: segmented sparse vs plain dense backward differ by {float(ratio.max()):.3e} of |ref| + rms"
    return ratio


def test_one_tile_with_a_long_list(hip):
    """600 faint splats on one tile, the segmented backward forced (as tests/test_segmented_backward.py forces it; it needs the
    free-running mode): the walk of that tile is cut in three, both launches run.  Against the unsegmented dense path, by that file's
    contract for segmented against plain: the compositing kernel's own quantities to 5e-5 of |ref| + rms, the gradients behind the
    covariance chain to the same in 99.5 % of the elements and 0.5 at most."""
    hip.set_deterministic(False)
    n = 600
    g = torch.Generator().manual_seed(5)
    means = torch.cat([(torch.rand(n, 2, generator=g) * 2 - 1) * 0.05 + torch.tensor([-0.8, -0.25]), (torch.rand(n, 1, generator=g) * 2 - 1) * 0.3], dim=1)
    scene = (means, torch.full((n, 3), 0.4) + 0.02 * torch.rand(n, 3, generator=g), torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=-1),
             torch.full((n, 1), 0.008), torch.randn(n, 16, 3, generator=g) * 0.3)

    def run(sparse, segmented):
        hip.SEGMENTED_BACKWARD = "always" if segmented else False
        out = _step(hip, scene, sparse=sparse, deg=3, split=False, adam=False, stale=sparse)
        count = hip.LAST_RASTER.get("segment_count")
        return out, (None if count is None else int(count.item()))

    got, count = run(True, True)
    ref, count_ref = run(False, False)
    assert count_ref is None and count is not None and count >= 2, f"the long tile published {count} segments beyond its first"
    assert got["grad_rows"] is not None and ref["grad_rows"] is None
    assert torch.equal(got["radii"], ref["radii"]) and float((got["render"] - ref["render"]).abs().max()) <= 2e-6
    assert torch.equal(got["grad_rows"], (got["packed"] != 0).any(dim=1).to(torch.uint8))
    for name in ("denom", "max_radii"):
        assert torch.equal(got[name], ref[name]), name
    for lo, hi, name, rel in ((0, 2, "dL/dmeans2d", 5e-5), (2, 5, "dL/dconic", 2e-5), (5, 6, "dL/dopacity", 2e-5), (6, 9, "dL/dcolour", 2e-5)):
        _close(got["packed"][:, lo:hi], ref["packed"][:, lo:hi], "compositing " + name, rel=rel)
    for name in ("viewspace", "opacities", "shs", "accum"):
        assert not torch.isnan(got[name]).any(), name
        _close(got[name], ref[name], name)
    for name in ("means", "scales", "rotations"):
        assert not torch.isnan(got[name]).any(), name
        a, b = got[name].double(), ref[name].double()
        ratio = (a - b).abs() / (b.abs() + float(b.pow(2).mean().sqrt()) + 1e-30)
        assert float((ratio <= 5e-5).double().mean()) >= 0.995 and float(ratio.max()) <= 0.5, (name, float(ratio.max()))

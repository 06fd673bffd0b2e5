"""The sparse tail of the fused Inria backward (`gspl_rasterize_inria_bwd_sparse`, `ops.SPARSE_TAIL`) and the Adam launch that does not
read a gradient it knows to be zero (`gspl_selective_adam_rows`), against the dense kernels (`ops.SPARSE_TAIL = False`) on identical
inputs, in the deterministic mode (the free-running compositing backward adds with float atomics and differs from run to run).

The contract is equality AS VALUES (`torch.equal`: -0.0 == +0.0) of every output of a step: all parameter gradients, the screen-space
gradient, the densification buffers, and parameters and both moments after `FusedAdam.step()`.  Where the dense kernels compute a zero
from a negative factor they write -0.0; the sparse ones leave the +0.0 of the cleared array.

Shapes: a 48 x 40 image (not a multiple of the 16-pixel tile) and N in {1, 255, 256, 257, 2000}: the block edges of the two per-splat
kernels (256 rows per workgroup), one workgroup and several.  The sparse scene (N = 2000) has ~200 large splats of opacity 0.99 in
front of the others: the cloud saturates and about one row in ten has a gradient (207 of 2000 in the fp64 oracle)."""
import numpy as np
import pytest
import torch

from oracle import gsplat_oracle as O

pytestmark = pytest.mark.gpu

W, H, FX = 48, 40, 60.0
BG = torch.tensor([0.25, 0.5, 0.125])
NAMES = ("means", "scales", "rotations", "opacities", "shs_dc", "shs_rest")


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib, ops
    _lib.lib()
    return ops


@pytest.fixture(autouse=True)
def _deterministic_and_restored(hip):
    was_det, was_sparse = hip.set_deterministic(True), hip.SPARSE_TAIL
    yield
    hip.set_deterministic(was_det)
    hip.SPARSE_TAIL = was_sparse


def _dev():
    return torch.device("cuda:0")


def _scene(n, deg, kind="sparse", seed=3):
    """sparse: a tenth of the splats (at most 200) large, opaque and in front, covering the image; the others behind them.
    faint: every splat in view and nearly transparent — nothing saturates, every row gets a gradient."""
    g = torch.Generator().manual_seed(seed)
    K = (deg + 1) ** 2
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    nf = min(200, max(n // 10, 1)) if n >= 10 else 0
    means, scales, opac = torch.empty(n, 3), torch.empty(n, 3), torch.empty(n, 1)
    means[:nf] = u(nf, 3) * torch.tensor([1.3, 1.1, 0.2]) + torch.tensor([0.0, 0.0, -1.0])
    scales[:nf] = 0.2 + 0.1 * torch.rand(nf, 3, generator=g)
    opac[:nf] = 0.99
    means[nf:] = u(n - nf, 3) * torch.tensor([1.8, 1.5, 0.4]) + torch.tensor([0.0, 0.0, 0.9])
    scales[nf:] = torch.exp(torch.randn(n - nf, 3, generator=g) * 0.5 - 3.0)
    opac[nf:] = torch.sigmoid(torch.randn(n - nf, 1, generator=g))
    if kind == "faint":
        means = u(n, 3) * torch.tensor([1.0, 0.8, 0.5])
        scales = 0.05 + 0.05 * torch.rand(n, 3, generator=g)
        opac = 0.02 + 0.03 * torch.rand(n, 1, generator=g)
    quats = torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=-1)
    shs = torch.randn(n, K, 3, generator=g) * 0.3
    return means, scales, quats, opac, shs


def _camera(shift=0.0):
    """The synthetic camera, moved sideways by `shift`: other splats leave the image and others come out from behind the front layer."""
    c = O.synthetic_camera(W, H, FX)
    if shift:
        proj = torch.linalg.inv(c["world_to_camera"]) @ c["full_projection"]
        w2c = c["world_to_camera"].clone()
        w2c[3, 0] = shift
        c = dict(c, world_to_camera=w2c, full_projection=w2c @ proj, camera_center=torch.linalg.inv(w2c)[3, :3])
    return c


def _settings(hip, cam, deg, accel=False):
    make = hip.AccelRasterizationSettings if accel else hip.GaussianRasterizationSettings
    return make(image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=BG.to(_dev()), scale_modifier=1.0,
                viewmatrix=cam["world_to_camera"].to(_dev()), projmatrix=cam["full_projection"].to(_dev()), sh_degree=deg,
                campos=cam["camera_center"].to(_dev()))


def _leaves(scene, raw, split):
    """The model's tensors as leaves on the GPU: (means, scales, rotations, opacities, shs | shs_dc, shs_rest)."""
    means, scales, quats, opac, shs = scene
    if raw:
        scales, opac, quats = torch.log(scales), torch.logit(opac), quats * 1.7
    ts = [means, scales, quats, opac] + ([shs[:, :1], shs[:, 1:]] if (split and shs.shape[1] > 1) else [shs])      # (degree 0: [N,1,3] alone)
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


def _render(hip, leaves, cam, deg, raw, aa=False, invd=False):
    m, s, q, o, *sh = leaves
    screen = torch.zeros_like(m, requires_grad=True)
    dc, rest = (sh[0], sh[1]) if len(sh) == 2 else (sh[0], None)
    if rest is not None and rest.shape[1] == 0:
        rest = None
    if aa or invd:
        render, radii, inv = hip.rasterize_inria_accel(_settings(hip, cam, deg, accel=True), m, screen, o, shs=dc, scales=s, rotations=q, shs_rest=rest,
                                                       raw_parameters=raw, antialiasing=aa, inverse_depth=invd)
    else:
        render, radii = hip.GaussianRasterizer(_settings(hip, cam, deg))(means3D=m, means2D=screen, opacities=o, shs=dc, shs_rest=rest, scales=s,
                                                                        rotations=q, raw_parameters=raw)
        inv = None
    return render, radii, inv, screen


def _step_outputs(hip, scene, *, sparse, deg, raw=False, split=True, aa=False, invd=False, v_zero=False, stale=False, cam=None):
    """One forward + backward with the densification statistics taken along; every output of the step as a dict of tensors."""
    from gspl_amd.density import request_stats_in_backward
    hip.SPARSE_TAIL = sparse
    leaves = _leaves(scene, raw, split)
    n = leaves[0].shape[0]
    g = torch.Generator().manual_seed(9)
    stats = [torch.rand(n, generator=g).to(_dev()), torch.randint(0, 5, (n,), generator=g).float().to(_dev()), (torch.rand(n, generator=g) * 5).to(_dev())]
    render, radii, inv, screen = _render(hip, leaves, cam or _camera(), deg, raw, aa, invd)
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
    out = {name: t.grad for name, t in zip(NAMES if len(leaves) == 6 else NAMES[:4] + ("shs",), leaves)}
    out["viewspace"] = screen.grad
    out.update(accum=stats[0], denom=stats[1], max_radii=stats[2], radii=radii, render=render.detach())
    tag = getattr(leaves[0].grad.untyped_storage(), "_gspl_grad_rows", None)
    out["grad_rows"] = None if tag is None else tag[0]
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
        if name == "grad_rows":
            continue
        g = got[name]
        assert not torch.isnan(g.float()).any(), f"{what}: NaN in {name}"
        assert torch.equal(r, g), f"{what}: {name} differs in {int((r != g).sum())} elements (max |diff| {float((r.float() - g.float()).abs().max()):.3e})"
    flags = got["grad_rows"]
    assert flags.dtype == torch.uint8 and flags.shape == (ref["means"].shape[0],) and int(flags.max()) <= 1
    missed = _nonzero_rows(ref) & (flags == 0)
    assert not bool(missed.any()), f"{what}: {int(missed.sum())} rows with a non-zero gradient carry flag 0"


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2000])
@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("split", [True, False])
def test_sparse_tail_equals_the_dense_kernels(hip, n, deg, raw, split):
    scene = _scene(n, deg)
    ref = _step_outputs(hip, scene, sparse=False, deg=deg, raw=raw, split=split)
    got = _step_outputs(hip, scene, sparse=True, deg=deg, raw=raw, split=split)
    _assert_same(ref, got, f"N={n} degree={deg} raw={raw} split={split}")
    if n == 2000:
        frac = float(_nonzero_rows(ref).float().mean())
        print(f"[sparse scene] rows with a non-zero reference gradient: {frac:.4f}; flagged: {float(got['grad_rows'].float().mean()):.4f}")
        assert 0.02 <= frac <= 0.50, f"the sparse scene is not sparse: {frac:.3f} of the rows have a gradient"


@pytest.mark.parametrize("aa,invd", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("raw", [False, True])
def test_sparse_tail_with_antialiasing_and_inverse_depth(hip, aa, invd, raw):
    scene = _scene(2000, 3)
    ref = _step_outputs(hip, scene, sparse=False, deg=3, raw=raw, aa=aa, invd=invd)
    got = _step_outputs(hip, scene, sparse=True, deg=3, raw=raw, aa=aa, invd=invd)
    _assert_same(ref, got, f"antialias={aa} invdepth={invd} raw={raw}")
    frac = float(_nonzero_rows(ref).float().mean())
    assert 0.02 <= frac <= 0.50, f"the sparse scene is not sparse: {frac:.3f} of the rows have a gradient"


def test_every_row_hit(hip):
    scene = _scene(2000, 3, kind="faint")
    ref = _step_outputs(hip, scene, sparse=False, deg=3)
    got = _step_outputs(hip, scene, sparse=True, deg=3)
    _assert_same(ref, got, "faint splats")
    frac = float(_nonzero_rows(ref).float().mean())
    assert frac > 0.9, f"the faint scene leaves {1 - frac:.3f} of the rows without a gradient"


def test_no_row_hit(hip):
    """v_out = 0: every gradient exactly zero, flags all 0, and the statistics still counted for the visible rows."""
    scene = _scene(2000, 3)
    ref = _step_outputs(hip, scene, sparse=False, deg=3, v_zero=True, cam=_camera(1.2))
    got = _step_outputs(hip, scene, sparse=True, deg=3, v_zero=True, cam=_camera(1.2))
    _assert_same(ref, got, "v_out = 0")
    assert not bool(_nonzero_rows(got).any()) and int(got["grad_rows"].sum()) == 0
    visible = got["radii"] > 0
    assert 0 < int(visible.sum()) < 2000
    g = torch.Generator().manual_seed(9)      # the buffers' start values, as _step_outputs draws them
    accum0, denom0, max0 = torch.rand(2000, generator=g).to(_dev()), torch.randint(0, 5, (2000,), generator=g).float().to(_dev()), (torch.rand(2000, generator=g) * 5).to(_dev())
    assert torch.equal(got["accum"], accum0) and torch.equal(got["denom"], denom0 + visible.float())
    assert torch.equal(got["max_radii"], torch.where(visible, torch.maximum(max0, got["radii"].float()), max0))


@pytest.mark.parametrize("n", [257, 2000])
def test_stale_memory_in_the_gradient_blocks(hip, n):
    """The gradient tensors come from `torch.empty`: blocks that held NaN a moment ago must come back cleared where no row is written."""
    scene = _scene(n, 3)
    ref = _step_outputs(hip, scene, sparse=False, deg=3, cam=_camera(1.2))
    got = _step_outputs(hip, scene, sparse=True, deg=3, stale=True, cam=_camera(1.2))
    _assert_same(ref, got, f"stale blocks, N={n}")


def test_precomputed_covariance_and_colours(hip):
    """v_cov3D and v_colors_precomp are among the arrays the sparse path clears."""
    n = 2000
    means, scales, quats, opac, shs = _scene(n, 0)
    g = torch.Generator().manual_seed(4)
    w, x, y, z = quats.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(n, 3, 3)
    M = R * scales[:, None, :]
    S = M @ M.transpose(1, 2)
    cov = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], dim=-1).contiguous()
    colours = torch.rand(n, 3, generator=g)
    outs = []
    for sparse in (False, True):
        hip.SPARSE_TAIL = sparse
        leaves = [t.clone().to(_dev()).requires_grad_(True) for t in (means, cov, opac, colours)]
        m, c6, o, cp = leaves
        screen = torch.zeros_like(m, requires_grad=True)
        render, radii = hip.GaussianRasterizer(_settings(hip, _camera(), 0))(means3D=m, means2D=screen, opacities=o, colors_precomp=cp, cov3D_precomp=c6)
        _poison_free_blocks(leaves)
        (render * _weights()).sum().backward()
        torch.cuda.synchronize()
        outs.append([t.grad for t in leaves] + [screen.grad])
    for name, r, g_ in zip(("means", "cov3D", "opacities", "colours", "viewspace"), *outs):
        assert not torch.isnan(g_).any(), name
        assert torch.equal(r, g_), f"{name} differs in {int((r != g_).sum())} elements"
    assert float((outs[0][1].reshape(n, -1) != 0).any(dim=1).float().mean()) < 0.5


# ---- Adam ------------------------------------------------------------------------------------------------------------------------------
LRS = (1.6e-4, 5e-3, 1e-3, 5e-2, 2.5e-3, 2.5e-3 / 20)


class _Model:
    def __init__(self, hip, sparse, monkeypatch_calls):
        from gspl_amd import optimizers
        self.hip, self.sparse, self.calls = hip, sparse, monkeypatch_calls
        self.leaves = _leaves(_scene(2000, 3), raw=False, split=True)
        self.opt = optimizers.FusedAdam([{"params": [t], "lr": lr, "name": name} for t, lr, name in zip(self.leaves, LRS, NAMES)], eps=1e-15)

    def backward(self, shift, retain=False):
        self.hip.SPARSE_TAIL = self.sparse
        render, _radii, _inv, _screen = _render(self.hip, self.leaves, _camera(shift), 3, False)
        loss = (render * _weights()).sum()
        loss.backward(retain_graph=retain)
        return loss

    def step(self):
        del self.calls[:]
        self.opt.step()
        torch.cuda.synchronize()
        assert len(self.calls) == 1, "one launch for the six tensors"
        return self.calls[0]

    def zero(self):
        for t in self.leaves:
            t.grad = None

    def state(self):
        out = {}
        for name, t in zip(NAMES, self.leaves):
            st = self.opt.state[t]
            out[name], out[name + ".exp_avg"], out[name + ".exp_avg_sq"] = t.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()
        return out


def _assert_states_equal(ref, got, what):
    for name, r in ref.items():
        g = got[name]
        assert not torch.isnan(g).any(), f"{what}: NaN in {name}"
        assert torch.equal(r, g), f"{what}: {name} differs in {int((r != g).sum())} elements (max |diff| {float((r - g).abs().max()):.3e})"


def test_adam_does_not_read_a_known_zero_gradient_and_falls_back(hip, monkeypatch):
    """Three steps over a view that changes (rows without a gradient in one frame carry moments from another): parameters and moments
    equal the dense path's after every step, with the row flags in use.  Then every way a gradient can stop being what the backward
    returned: the flags must not be used, and the result still equals the dense path's."""
    from gspl_amd import _lib
    calls = []
    real_call = _lib.call

    def spy(name, *args):
        if name in ("gspl_selective_adam_limited", "gspl_selective_adam_rows"):
            calls.append(name == "gspl_selective_adam_rows" and args[4] is not None)      # the grad_rows argument
        return real_call(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    ref, got = _Model(hip, False, calls), _Model(hip, True, calls)

    def both(fn, expect_flags, what):
        states = []
        for model in (ref, got):
            model.zero()
            fn(model)
            used = model.step()
            assert used == (expect_flags and model.sparse), f"{what}: row flags {'not ' if not used else ''}used on the {'sparse' if model.sparse else 'dense'} path"
            states.append(model.state())
        _assert_states_equal(states[0], states[1], what)

    for k, shift in enumerate((0.0, 1.2, 0.0)):
        both(lambda model: model.backward(shift), True, f"step {k + 1}")
    zero_moment_rows = (ref.state()["shs_rest.exp_avg"].reshape(2000, -1) == 0).all(dim=1)
    flags = got.leaves[5].grad.untyped_storage()._gspl_grad_rows[0]
    assert bool(((flags == 0) & ~zero_moment_rows).any()), "no row without a gradient in this frame carries moments from another"
    assert bool(((flags == 0) & zero_moment_rows).any()) and bool((flags == 1).any())

    def accumulated(model):
        model.backward(0.0)
        model.backward(1.2)
    both(accumulated, False, "two backwards accumulated into one .grad")

    def edited(model):
        model.backward(1.2)
        rest = model.leaves[5].grad
        row = int((~(rest.reshape(2000, -1) != 0).any(dim=1)).nonzero()[0])      # a row without a gradient: flag 0 on the sparse path
        for t in model.leaves:
            t.grad[7] = 1
        rest[row] = 1
    both(edited, False, "p.grad[7] = 1 written in place")

    def cloned(model):
        model.backward(0.0)
        for t in model.leaves:
            t.grad = t.grad.clone()
    both(cloned, False, "p.grad replaced by a clone")

    def retained(model):
        hip.SPARSE_TAIL = model.sparse
        render, _radii, _inv, _screen = _render(hip, model.leaves, _camera(1.2), 3, False)
        loss = (render * _weights()).sum()
        loss.backward(retain_graph=True)
        loss.backward()
    both(retained, False, "a second backward through retain_graph")

    both(lambda model: model.backward(0.0), True, "a plain step after the fall-backs")


def test_sparse_scene_against_the_oracle(hip):
    """The sparse scene's gradients, sparse tail on, free-running, against the fp64 oracle at the tolerances of
    tests/test_hip_parity.py::test_end_to_end_inria_api."""
    from hip_helpers import assert_pipeline_attributed
    hip.set_deterministic(False)
    hip.SPARSE_TAIL = True
    means, scales, quats, opac, shs = _scene(2000, 3)
    cam = _camera()
    wimg = torch.randn(3, H, W, generator=torch.Generator().manual_seed(1))
    leaves = [t.clone().to(_dev()).requires_grad_(True) for t in (means, scales, quats, opac, shs)]
    m, s, q, o, c = leaves
    screen = torch.zeros_like(m, requires_grad=True)
    render, radii = hip.GaussianRasterizer(_settings(hip, cam, 3))(means3D=m, means2D=screen, opacities=o, shs=c, scales=s, rotations=q)
    (render * wimg.to(_dev())).sum().backward()
    assert getattr(m.grad.untyped_storage(), "_gspl_grad_rows", None) is not None
    dl = [t.double().requires_grad_(True) for t in (means, scales, quats, opac, shs)]
    r = O.render_inria(*dl, 3, cam["world_to_camera"].double(), cam["full_projection"].double(), cam["camera_center"].double(),
                       cam["tanfovx"], cam["tanfovy"], W, H, BG.double())
    (r["render"] * wimg.double()).sum().backward()
    assert np.mean(radii.cpu().numpy() == r["radii"].numpy()) > 0.999
    ref_ndc = r["xy"].grad.numpy() * np.array([0.5 * W, 0.5 * H])
    assert_pipeline_attributed(O.MODE_INRIA, r, W, H, BG.double(), render.detach().cpu().numpy(),
                               [(name, got.grad.cpu().numpy(), ref.grad.numpy()) for got, ref, name in zip(leaves, dl, ("means", "scales", "quats", "opacities", "shs"))]
                               + [("viewspace_points.grad", screen.grad[:, :2].cpu().numpy(), ref_ndc)], opacities=dl[3], gpu_radii=radii)
    assert torch.all(screen.grad[:, 2] == 0)

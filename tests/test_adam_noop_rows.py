"""`selective_adam_kernel` passes over 16-byte chunks whose moments are +0 and whose gradient is zero without loading the parameter or
storing anything (csrc/adam.hip).  The contract is BIT equality with the dense update — the same library with `GSPL_ADAM_SKIP_NOOP=0`,
which the native code reads once: parameters and both moments as int32 views, `torch.equal`.

The dense results come from ONE child process (this file run as a script with the switch off) that computes every case below from the
same seeds and saves them; the tests compute the cases in this process and compare.

Shapes: N = 4099 and 257 rows, row widths 1, 3, 4, 45 (the model's) and 32, 33 (either side of `GSPL_ADAM_ROWS_MIN`), all six in one
launch; no total but the 4- and 32-wide ones is a multiple of 4.  Row kinds, mixed at random with runs of never-touched rows long enough for whole
128-byte lines to be dead: never touched; a gradient in step 1 only (the moments then decay and must keep moving); a gradient every
step; g = -0.0 (flagged as a gradient row and not); moments of -0.0 (the dense kernel rewrites them to +0.0); p of -0.0, a denormal,
inf and NaN over zero moments and a zero gradient."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SWITCH = "GSPL_ADAM_SKIP_NOOP"
WIDTHS = (1, 3, 4, 45, 32, 33)
LRS = (5e-2, 1.6e-4, 1e-3, 1.25e-4, 2.5e-3, 5e-3)
NEVER, ONCE, ALWAYS, NEG_G_FLAGGED, NEG_G, NEG_MOMENTS, ODD_P = range(7)
KIND_WEIGHTS = torch.tensor([0.0, 0.08, 0.08, 0.04, 0.04, 0.06, 0.10])     # (NEVER: the runs below)
SNAPSHOTS = (1, 2, 5)


def _dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().clone()


def _row_kinds(n, g):
    """A kind per row: runs of 1 - 12 NEVER rows between single rows of the other kinds."""
    kinds = torch.full((n,), NEVER, dtype=torch.int64)
    r = int(torch.randint(0, 4, (1,), generator=g))
    while r < n:
        kinds[r] = int(torch.multinomial(KIND_WEIGHTS, 1, generator=g))
        r += 1 + int(torch.randint(0, 13, (1,), generator=g))
    return kinds


def _tensors(n, kinds, g):
    """[(p, m, v)] on the CPU for every width of WIDTHS."""
    odd = torch.tensor([-0.0, 1e-41, float("inf"), float("nan"), -1e-39, float("-inf")])
    out = []
    for w in WIDTHS:
        p = torch.randn(n, w, generator=g)
        m, v = torch.zeros(n, w), torch.zeros(n, w)
        rows = (kinds == ODD_P).nonzero().flatten()
        p[rows] = odd[(torch.arange(w)[None, :] + rows[:, None]) % len(odd)]
        rows = (kinds == NEG_MOMENTS).nonzero().flatten()
        which = (torch.arange(w)[None, :] + rows[:, None]) % 3          # m alone, v alone, both
        m[rows] = torch.where(which != 1, -0.0, 0.0)
        v[rows] = torch.where(which != 0, -0.0, 0.0)
        out.append((p, m, v))
    return out


def _grad(n, w, kinds, step, g):
    grad = torch.zeros(n, w)
    live = (kinds == ALWAYS) | ((kinds == ONCE) & (step == 1))
    grad[live] = torch.randn(int(live.sum()), w, generator=g)
    grad[(kinds == NEG_G_FLAGGED) | (kinds == NEG_G)] = -0.0
    return grad


def _launch(L, items, n, vis, rows, b1, b2, eps, bc1, bc2s):
    table = (L.AdamTensor * len(items))()
    for k, (p, g, m, v, lr, w) in enumerate(items):
        table[k] = L.AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), lr, w)
    L.call("gspl_selective_adam_rows", len(items), table, n, L.ptr(vis), L.ptr(rows), float(b1), float(b2), float(eps), float(bc1), float(bc2s), 0, L.stream())


def _mixed(n, use_rows, use_vis, seed, steps=5, hyper=None, lrs=LRS):
    """`steps` launches over the six tensors; {f"{width}/{name}@{step}": int32 bits} at the steps of SNAPSHOTS.
    hyper: step -> (b1, b2, eps, bias_correction1, bias_correction2_sqrt), default torch.optim.Adam's at eps 1e-15."""
    from gspl_amd import _lib as L
    g = torch.Generator().manual_seed(seed)
    kinds = _row_kinds(n, g)
    state = [[t.to(_dev()) for t in pmv] for pmv in _tensors(n, kinds, g)]
    vis = (torch.rand(n, generator=g) < 0.7).to(torch.uint8).to(_dev()) if use_vis else None
    out = {}
    for step in range(1, steps + 1):
        grads = [_grad(n, w, kinds, step, g).to(_dev()) for w in WIDTHS]
        live = (kinds == ALWAYS) | ((kinds == ONCE) & (step == 1)) | (kinds == NEG_G_FLAGGED)
        rows = live.to(torch.uint8).to(_dev()) if use_rows else None
        b1, b2, eps, bc1, bc2s = hyper(step) if hyper else (0.9, 0.999, 1e-15, 1 - 0.9 ** step, (1 - 0.999 ** step) ** 0.5)
        _launch(L, [(p, gr, m, v, lr, w) for (p, m, v), gr, lr, w in zip(state, grads, lrs, WIDTHS)], n, vis, rows, b1, b2, eps, bc1, bc2s)
        if step in SNAPSHOTS:
            for (p, m, v), w in zip(state, WIDTHS):
                out.update({f"{w}/p@{step}": _bits(p), f"{w}/m@{step}": _bits(m), f"{w}/v@{step}": _bits(v)})
    return out


def _boundary(use_rows):
    """Row width 45: most 16-byte chunks that touch two rows straddle a live and a dead one, in both orders; the last row is dead, so the
    flag of the second row of the last straddling chunk is the last byte of `grad_rows`."""
    from gspl_amd import _lib as L
    live = torch.tensor([1, 0, 1, 0, 0, 1, 1, 0], dtype=torch.bool)
    n, w = live.numel(), 45
    g = torch.Generator().manual_seed(11)
    p, m, v = torch.randn(n, w, generator=g).to(_dev()), torch.zeros(n, w, device=_dev()), torch.zeros(n, w, device=_dev())
    rows = live.to(torch.uint8).to(_dev()) if use_rows else None
    out = {}
    for step in (1, 2):
        grad = torch.zeros(n, w)
        grad[live] = torch.randn(int(live.sum()), w, generator=g)
        _launch(L, [(p, grad.to(_dev()), m, v, 1e-2, w)], n, None, rows, 0.9, 0.999, 1e-15, 1 - 0.9 ** step, (1 - 0.999 ** step) ** 0.5)
        out.update({f"p@{step}": _bits(p), f"m@{step}": _bits(m), f"v@{step}": _bits(v)})
    return out


# hyper-parameters outside the range in which a zero chunk is a no-op: the launch takes the dense path whole
GUARDS = {
    "eps=0": dict(hyper=lambda s: (0.9, 0.999, 0.0, 1 - 0.9 ** s, (1 - 0.999 ** s) ** 0.5)),                        # 0 / 0: NaN parameters
    "lr<0": dict(lrs=(5e-2, 1.6e-4, 1e-3, -1.25e-4, 2.5e-3, 5e-3)),                                                  # p - (-0): -0.0 becomes +0.0
    "lr=-0": dict(lrs=(5e-2, 1.6e-4, 1e-3, -0.0, 2.5e-3, 5e-3)),
    "1/bc2=inf": dict(hyper=lambda s: (0.9, 0.999, 1e-15, 1 - 0.9 ** s, 1e-45)),                                    # 0 * inf: NaN
    "1/bc1=inf": dict(hyper=lambda s: (0.9, 0.999, 1e-15, 1e-45, (1 - 0.999 ** s) ** 0.5)),                          # inf * 0: NaN
}


def _whole_path():
    """Three training steps of one 128 x 96 frame (N = 20 000, a front layer of opaque splats hides most of the cloud) through the
    Inria rasterizer's fused call and `FusedAdam`, deterministic mode; parameters and moments of the six groups."""
    import gspl_amd  # noqa: F401
    from gspl_amd import ops, synthetic
    from gspl_amd.optimizers import FusedAdam
    W, H, n, front = 128, 96, 20_000, 250
    was = ops.set_deterministic(True)
    try:
        g = torch.Generator().manual_seed(5)
        means, scales, quats, opac, shs = synthetic.scene(n, seed=42)
        means[:front] = torch.cat([(torch.rand(front, 2, generator=g) * 2 - 1) * 1.4, -1.6 + 0.1 * torch.rand(front, 1, generator=g)], dim=1)
        scales[:front], opac[:front] = 0.25, 0.9
        cam = synthetic.camera(W, H, 100.0)
        leaves = [t.clone().contiguous().to(_dev()).requires_grad_(True) for t in (means, scales, quats, opac, shs[:, :1], shs[:, 1:])]
        names = ("means", "scales", "rotations", "opacities", "shs_dc", "shs_rest")
        opt = FusedAdam([{"params": [t], "lr": lr, "name": nm} for t, lr, nm in zip(leaves, (1.6e-4, 5e-3, 1e-3, 5e-2, 2.5e-3, 1.25e-4), names)], eps=1e-15)
        settings = ops.GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=torch.tensor([0.25, 0.5, 0.125]).to(_dev()),
            scale_modifier=1.0, viewmatrix=cam["world_to_camera"].to(_dev()), projmatrix=cam["full_projection"].to(_dev()), sh_degree=3,
            campos=cam["camera_center"].to(_dev()))
        target = torch.rand(3, H, W, generator=g).to(_dev())
        m, s, q, o, dc, rest = leaves
        for _ in range(3):
            screen = torch.zeros_like(m, requires_grad=True)
            render, _radii = ops.GaussianRasterizer(settings)(means3D=m, means2D=screen, opacities=o, shs=dc, shs_rest=rest, scales=s, rotations=q)
            (render - target).abs().mean().backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
        out = {}
        for nm, t in zip(names, leaves):
            out.update({f"{nm}/p": _bits(t), f"{nm}/m": _bits(opt.state[t]["exp_avg"]), f"{nm}/v": _bits(opt.state[t]["exp_avg_sq"])})
        return out
    finally:
        ops.set_deterministic(was)


MIXED = [(n, use_rows, use_vis) for n in (4099, 257) for use_rows in (False, True) for use_vis in (False, True)]
CASES = {f"mixed-{n}-rows{int(r)}-vis{int(v)}": (lambda n=n, r=r, v=v: _mixed(n, r, v, seed=100 + n)) for n, r, v in MIXED}
CASES.update({f"boundary-rows{int(r)}": (lambda r=r: _boundary(r)) for r in (False, True)})
CASES.update({f"guard-{k}": (lambda kw=kw: _mixed(257, False, False, seed=7, steps=2, **kw)) for k, kw in GUARDS.items()})
CASES["whole-path"] = _whole_path


@pytest.fixture(scope="module")
def dense(tmp_path_factory):
    """{case: its result} from a process in which the library never skips a chunk."""
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert os.environ.get(SWITCH, "1") != "0", f"{SWITCH}=0: this process would compare the dense update with itself"
    path = str(tmp_path_factory.mktemp("adam_dense") / "dense.pt")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, **{SWITCH: "0"}), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(path)


def _same(got, ref, what):
    assert sorted(got) == sorted(ref)
    for k in got:
        assert torch.equal(got[k], ref[k]), f"{what}: {k} differs from the dense update in {int((got[k] != ref[k]).sum())} of {got[k].numel()} words"


@pytest.mark.parametrize("case", [c for c in CASES if c.startswith("mixed") or c.startswith("boundary")])
def test_bits_equal_the_dense_update(dense, case):
    got = CASES[case]()
    _same(got, dense[case], case)
    if case.startswith("mixed"):
        # the case holds what it is meant to hold: rows that stay zero, moments that were -0.0 and are +0.0 now, NaN and inf kept
        assert bool((got["45/v@5"].view(-1, 45) == 0).all(dim=1).any()) and bool((got["45/v@5"] != 0).any())
        assert not bool((got["45/m@1"] == -2 ** 31).any()) or "vis1" in case
        p = got["45/p@5"].view(torch.float32)
        assert bool(torch.isnan(p).any()) and bool(torch.isinf(p).any())


@pytest.mark.parametrize("guard", list(GUARDS))
def test_outside_the_safe_range_the_dense_path_runs(dense, guard):
    got = CASES["guard-" + guard]()
    _same(got, dense["guard-" + guard], guard)


def test_the_guarded_launches_differ_from_a_skipping_one(dense):
    """What the guard is for: with eps = 0 a never-touched row becomes NaN in the dense update, with lr < 0 a parameter of -0.0 becomes
    +0.0 — a launch that skipped those rows would have kept them."""
    nan_before = int(torch.isnan(dense["guard-lr<0"]["45/p@1"].view(torch.float32)).sum())
    for guard in ("eps=0", "1/bc2=inf", "1/bc1=inf"):
        assert int(torch.isnan(dense["guard-" + guard]["45/p@1"].view(torch.float32)).sum()) > nan_before, guard
    g = torch.Generator().manual_seed(7)
    kinds = _row_kinds(257, g)
    p0 = _tensors(257, kinds, g)[3][0]
    neg_zero = (p0.view(torch.int32) == -2 ** 31) & (kinds == ODD_P)[:, None]
    assert bool(neg_zero.any()) and bool((dense["guard-lr<0"]["45/p@1"].view(257, 45)[neg_zero] == 0).all())


def test_whole_path_equals_the_dense_update(dense):
    got = _whole_path()
    _same(got, dense["whole-path"], "fused Inria call + FusedAdam, three steps")
    v = got["shs_rest/v"].view(20_000, -1)
    dead = int((v == 0).all(dim=1).sum())
    print(f"rows of shs_rest that never had a gradient: {dead} of 20000")
    assert 0 < dead < 20_000


@pytest.mark.parametrize("last_row_only", [False, True])
def test_a_dead_row_and_the_bands_around_it_stay_as_they_are(monkeypatch, last_row_only):
    """p, m and v carved out of larger blocks with a poisoned band on either side (tests/test_guard_bands_staged.py): every row dead,
    and every row live but the last, which ends where the upper band begins."""
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from test_guard_bands_staged import Guards
    from gspl_amd import _lib as L
    L.lib()
    guards = Guards(monkeypatch)
    n, w = 257, 45
    g = torch.Generator().manual_seed(3)
    host = torch.randn(n, w, generator=g)
    host[-1, :6] = torch.tensor([-0.0, 1e-41, float("inf"), float("nan"), -1e-39, float("-inf")])
    p, m, v = torch.empty((n, w), device=_dev()), torch.zeros((n, w), device=_dev()), torch.zeros((n, w), device=_dev())
    assert len(guards.blocks) == 3
    p.copy_(host)
    live = torch.zeros(n, dtype=torch.bool)
    if last_row_only:
        live[:-1] = True
    grad = torch.zeros(n, w)
    grad[live] = torch.randn(int(live.sum()), w, generator=g)
    grad = grad.to(_dev())
    before = [_bits(t) for t in (p, m, v)]
    for rows in (None, live.to(torch.uint8).to(_dev())):
        _launch(L, [(p, grad, m, v, 1e-2, w)], n, None, rows, 0.9, 0.999, 1e-15, 0.1, 0.03)
    after = [_bits(t) for t in (p, m, v)]
    assert guards.check("selective_adam") == 3
    dead = ~live
    for b, a, name in zip(before, after, "pmv"):
        assert torch.equal(b[dead], a[dead]), name
        assert not last_row_only or not torch.equal(b[live], a[live]), name


if __name__ == "__main__":
    assert os.environ.get(SWITCH) == "0"
    sys.path.insert(0, ROOT)
    import gspl_amd  # noqa: F401
    torch.save({name: fn() for name, fn in CASES.items()}, sys.argv[1])

"""The bilateral-grid route without a GPU: the fp64 oracle against torch's fp64 `grid_sample` (border and exact-border gradient
conventions included), the `fused_bilagrid` stand-in, the launcher's `LambdaLR` shim, and — with the reference tree present — the
reference's unedited `BilagridProcessor` (default `fused=True`) and `FreezeBilagrid` plugin on oracle ops substituted through the
stand-in's late binding, checked against the reference's own `lib_bilagrid`."""
import os
import subprocess
import sys
import textwrap
import types

import pytest
import torch
import torch.nn.functional as F

import bilagrid_oracle as BO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_ROOT = os.environ.get("GSPL_REFERENCE_ROOT", "/root/reference")
REF_PROCESSOR = os.path.join(REF_ROOT, "internal", "output_processors", "bilagrid.py")
needs_reference = pytest.mark.skipif(not os.path.exists(REF_PROCESSOR), reason="reference tree not present")


def _grid_sample_slice(grids, xy, rgb, idx):
    """lib_bilagrid's formulation (restated): grid_sample(bilinear, align_corners, border) then the affine."""
    B, H, W, _ = rgb.shape
    gray = rgb @ torch.tensor(BO.GRAY, dtype=rgb.dtype)
    coords = torch.cat([(xy.expand(B, H, W, 2) - 0.5) * 2, (gray * 2 - 1).unsqueeze(-1)], dim=-1).unsqueeze(1)
    A = F.grid_sample(grids[list(idx)], coords, mode="bilinear", align_corners=True, padding_mode="border")
    A = A.squeeze(2).permute(0, 2, 3, 1)
    return BO.apply_affine(A, rgb)


def _inputs(seed, B=2, H=7, W=9, gx=6, gy=5, gw=4, n=3):
    g = torch.Generator().manual_seed(seed)
    grids = BO.identity_grids(n, gx, gy, gw) + 0.3 * torch.randn(n, 12, gw, gy, gx, generator=g, dtype=torch.float64)
    rgb = -0.3 + 1.6 * torch.rand(B, H, W, 3, generator=g, dtype=torch.float64)
    rgb[:, 0, 0] = 0.0                          # gray exactly 0: w on the lower bound
    rgb[:, 0, 1] = 1.5                          # beyond the upper bound
    rgb[:, 0, 2] = torch.tensor([0.5, 0.5, 0.5], dtype=torch.float64)   # w = 1.5 (L = 4): inside
    xy = torch.rand(B, H, W, 2, generator=g, dtype=torch.float64)
    xy[:, 1, 0] = torch.tensor([0.0, 1.0], dtype=torch.float64)         # the xy borders
    xy[:, 1, 1] = torch.tensor([1.0, 0.0], dtype=torch.float64)
    return grids, xy, rgb


def test_oracle_matches_grid_sample_forward_and_gradients():
    grids, xy, rgb = _inputs(1)
    idx = [2, 0]
    dout = torch.randn(rgb.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    out, dg, dc, terms = BO.slice_grads(grids, xy, rgb, idx, dout)
    g = grids.clone().requires_grad_(True)
    c = rgb.clone().requires_grad_(True)
    ref = _grid_sample_slice(g, xy, c, idx)
    rg, rc = torch.autograd.grad((ref * dout).sum(), (g, c))
    assert torch.allclose(out, ref.detach(), rtol=0, atol=1e-12)
    assert torch.allclose(dg, rg, rtol=0, atol=1e-12) and torch.allclose(dc, rc, rtol=0, atol=1e-12)
    assert bool((terms >= dg.abs() - 1e-12).all()) and float(terms[1].abs().sum()) == 0.0


def test_oracle_border_convention_matches_grid_sample():
    """d out / d rgb through the guidance is 0 at w = 0, at w = L - 1 and beyond, as torch's grid_sample has it."""
    grids = BO.identity_grids(1, 3, 3, 5) + 0.2 * torch.randn(1, 12, 5, 3, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    xy = torch.full((1, 1, 3, 2), 0.3, dtype=torch.float64)
    # gray exactly 0 (w on the lower bound), and beyond either bound.  (Gray of (1, 1, 1) lands on either side of 1 in fp64 depending
    # on the order of the sum: not a case that can pin a convention.)
    rgb = torch.tensor([[[[0.0, 0.0, 0.0], [2.0, 2.0, 2.0], [-1.0, -1.0, -1.0]]]], dtype=torch.float64)
    dout = torch.ones_like(rgb)
    _, _, dc, _ = BO.slice_grads(grids, xy, rgb, [0], dout)
    c = rgb.clone().requires_grad_(True)
    rc, = torch.autograd.grad((_grid_sample_slice(grids, xy, c, [0]) * dout).sum(), (c,))
    assert torch.allclose(dc, rc, atol=1e-12)
    # at those pixels only the affine part remains: dc_j = sum_i dout_i A_{4i+j}
    A = BO.affine(grids, xy, rgb, [0])
    direct = A.reshape(1, 1, 3, 3, 4)[..., :3].sum(-2)
    assert torch.allclose(dc, direct, atol=1e-12)


def test_tv_oracle_matches_lib_bilagrid_formulation():
    x = torch.randn(3, 12, 4, 5, 6, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    tv = 0
    for i in range(2, 5):
        n = x.shape[i]
        x1, x2 = x.index_select(i, torch.arange(1, n)), x.index_select(i, torch.arange(0, n - 1))
        tv = tv + (x1 - x2).pow(2).sum() / max(x1[0].numel(), 1)
    assert abs(float(BO.tv(x)) - float(tv / 3)) <= 1e-12 * float(tv)
    y = torch.randn(2, 12, 1, 3, 1, dtype=torch.float64)          # sizes of 1: those terms are 0
    assert abs(float(BO.tv(y)) - float((y[:, :, :, 1:] - y[:, :, :, :-1]).pow(2).sum() / (12 * 2) / 2)) < 1e-12


def test_fused_bilagrid_stand_in_is_registered():
    import gspl_amd  # noqa: F401
    from gspl_amd import compat
    compat.install()
    import fused_bilagrid
    if "gspl_amd" not in (fused_bilagrid.__doc__ or ""):
        pytest.skip("a real fused_bilagrid package is installed")
    from fused_bilagrid import BilateralGrid, slice, total_variation_loss  # noqa: F401
    bg = BilateralGrid(num=2, grid_X=4, grid_Y=3, grid_W=2)
    assert tuple(bg.grids.shape) == (2, 12, 2, 3, 4) and set(bg.state_dict()) == {"grids", "rgb2gray_weight"}
    ident = torch.tensor([1., 0, 0, 0, 0, 1., 0, 0, 0, 0, 1., 0])
    assert torch.equal(bg.grids[1, :, 1, 2, 3].detach(), ident)
    with pytest.raises(RuntimeError, match="GPU only"):
        slice(bg, torch.zeros(1, 3, 4, 2), torch.zeros(1, 3, 4, 3), torch.zeros(1, 1, dtype=torch.long))
    with pytest.raises(RuntimeError, match="GPU only"):
        total_variation_loss(bg.grids)
    with pytest.raises(NotImplementedError):
        bg(torch.zeros(1, 2), torch.zeros(1, 3))
    with pytest.raises(NotImplementedError):
        slice(bg, torch.zeros(5, 2), torch.zeros(5, 3), torch.zeros(5, 1, dtype=torch.long))


_LAUNCHED = textwrap.dedent("""
    import json, sys, torch
    from torch.optim import lr_scheduler
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    s = torch.optim.lr_scheduler.LambdaLR(optimizer=opt, lr_lambda=lambda i: 0.5, verbose=False)
    s.step()
    print(json.dumps({"lr": opt.param_groups[0]["lr"], "is_lrscheduler": isinstance(s, lr_scheduler.LRScheduler)}))
""")


def test_launcher_lets_lambdalr_take_verbose(tmp_path):
    script = tmp_path / "uses_verbose.py"
    script.write_text(_LAUNCHED)
    probe = textwrap.dedent(f"""
        import sys, inspect
        sys.path.insert(0, {ROOT!r})
        import torch
        from torch.optim import lr_scheduler
        before = lr_scheduler.LambdaLR
        import gspl_amd, gspl_amd.renderers
        from gspl_amd import compat
        compat.install()
        assert lr_scheduler.LambdaLR is before, "importing the package must not patch torch"
        from gspl_amd import launch
        launch.main([{str(script)!r}])
    """)
    r = subprocess.run([sys.executable, "-c", probe], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    assert '"lr": 0.5' in line and '"is_lrscheduler": true' in line


def _stub_tensorly():
    if "tensorly" in sys.modules:
        return
    tl = types.ModuleType("tensorly")
    tl.set_backend = lambda name: None
    dec = types.ModuleType("tensorly.decomposition")

    def parafac(*a, **k):
        raise NotImplementedError("tensorly stand-in: only the import is provided")
    dec.parafac = parafac
    tl.decomposition = dec
    sys.modules["tensorly"] = tl
    sys.modules["tensorly.decomposition"] = dec


def _reference_modules():
    if REF_ROOT not in sys.path:
        sys.path.insert(0, REF_ROOT)
    _stub_tensorly()
    import importlib
    proc = importlib.import_module("internal.output_processors.bilagrid")
    lib = importlib.import_module("internal.utils.lib_bilagrid")
    freeze = importlib.import_module("internal.plugins.freeze_bilagrid")
    return proc, lib, freeze


def _oracle_ops(monkeypatch):
    """The stand-in binds its names at call time: substitute the fp64 oracle for the HIP ops (CPU)."""
    import gspl_amd  # noqa: F401
    from gspl_amd import bilagrid, compat
    compat.install()

    def oracle_slice(bil_grids, xy, rgb, grid_idx):
        B = rgb.shape[0]
        gi = grid_idx.reshape(-1)
        idx = [int(gi[0])] * B if gi.numel() == 1 else [int(v) for v in grid_idx.reshape(B, -1)[:, 0]]
        return {"rgb": BO.slice(bil_grids.grids.double(), xy.double(), rgb.double(), idx).float()}
    monkeypatch.setattr(bilagrid, "slice", oracle_slice)
    monkeypatch.setattr(bilagrid, "total_variation_loss", lambda x: BO.tv(x.double()).float())


@needs_reference
def test_reference_processor_runs_unedited_on_the_stand_in(monkeypatch):
    from torch.optim import lr_scheduler
    monkeypatch.setattr(lr_scheduler, "LambdaLR", lr_scheduler.LambdaLR)       # restored after the test
    from gspl_amd import launch
    launch.accept_lambdalr_verbose()
    _oracle_ops(monkeypatch)
    proc_mod, lib, freeze_mod = _reference_modules()
    cfg = proc_mod.BilagridProcessor()
    assert cfg.fused is True
    proc = cfg.instantiate()
    dataparser = types.SimpleNamespace(appearance_group_ids={"a": [0, 0.0], "b": [2, 1.0], "c": [1, 0.5]})
    pl_module = types.SimpleNamespace(device=torch.device("cpu"), extra_train_metrics=[], on_after_backward_hooks=[],
                                      trainer=types.SimpleNamespace(datamodule=types.SimpleNamespace(dataparser_outputs=dataparser)))
    proc.setup("fit", pl_module)
    assert tuple(proc.bgrid.grids.shape) == (3, 12, 8, 16, 16)
    optimizer, scheduler = proc.training_setup(pl_module)
    assert pl_module.extra_train_metrics == [proc.tv_loss]
    with torch.no_grad():
        proc.bgrid.grids.add_(0.2 * torch.randn(proc.bgrid.grids.shape, generator=torch.Generator().manual_seed(5)))
    H, W = 11, 14
    render = torch.rand(3, H, W, generator=torch.Generator().manual_seed(6))
    camera = types.SimpleNamespace(height=H, width=W, device=torch.device("cpu"), appearance_id=torch.tensor(2))
    outputs = {"render": render.clone()}
    proc(camera, outputs)
    got = outputs["render"]
    assert tuple(got.shape) == (3, H, W)
    # the reference's own lib_bilagrid on the same grids
    ref_grid = lib.BilateralGrid(3)
    ref_grid.load_state_dict({k[len("bgrid."):]: v for k, v in proc.state_dict().items()})
    ref = lib.slice(ref_grid, proc.build_grid_xy(camera).unsqueeze(0), render.permute(1, 2, 0).unsqueeze(0),
                    camera.appearance_id[None, None])["rgb"].squeeze(0).permute(2, 0, 1)
    assert torch.allclose(got, ref, atol=2e-6)
    metrics, pbar = {"loss": torch.tensor(0.0)}, {}
    proc.tv_loss(outputs, None, None, 0, pl_module, metrics, pbar)
    assert abs(float(metrics["tv"]) - 10 * float(lib.total_variation_loss(ref_grid.grids))) <= 1e-5 * float(metrics["tv"]) + 1e-9
    # checkpoints: the same key set both ways
    assert set(proc.state_dict()) == {"bgrid.grids", "bgrid.rgb2gray_weight"}
    assert {"bgrid." + k for k in lib.BilateralGrid(3).state_dict()} == set(proc.state_dict())
    fresh = cfg.instantiate()
    fresh.load_state_dict(proc.state_dict())
    assert torch.equal(fresh.bgrid.grids, proc.bgrid.grids)
    # FreezeBilagrid drops the grids' gradient after every backward
    plugin = freeze_mod.FreezeBilagrid().instantiate()
    pl_module.output_processor = proc
    plugin.setup(pl_module)
    proc.bgrid.grids.grad = torch.ones_like(proc.bgrid.grids)
    for hook in pl_module.on_after_backward_hooks:
        hook(None, None, None, 0, pl_module)
    assert proc.bgrid.grids.grad is None
    assert isinstance(scheduler, lr_scheduler.LRScheduler) and optimizer.param_groups[0]["eps"] == 1e-15


def test_oracle_against_the_reference_fixture(golden_dir):
    """tests/golden/ref_bilagrid.npz: the reference's lib_bilagrid (fp32, CPU) on seeded cases.  Bounds: fp32 against fp64;
    a colour gradient whose guidance lies within a few ulps of a level may take either one-sided difference."""
    import numpy as np
    z = np.load(os.path.join(golden_dir, "ref_bilagrid.npz"))
    U = 2.0 ** -24
    cases = sorted({k.split("_")[0] for k in z.files if k.startswith("c")})
    assert len(cases) == 4
    for c in cases:
        t = lambda name: torch.from_numpy(z[f"{c}_{name}"]).double()
        grids, xy, rgb, dout = t("grids"), t("xy"), t("rgb"), t("dout")
        B = rgb.shape[0]
        gi = z[f"{c}_idx"].reshape(-1)
        idx = [int(gi[0])] * B if gi.size == 1 else [int(v) for v in z[f"{c}_idx"].reshape(B, -1)[:, 0]]
        out, dg, dc, terms = BO.slice_grads(grids, xy, rgb, idx, dout)
        ref = t("out")
        assert float(((out - ref).abs() / (1 + ref.abs())).max()) <= 1e-5, c
        touch = BO.touch_terms(grids, xy, rgb, idx, dout)
        bound = 1e-4 * terms + 16 * U * max(grids.shape[2:]) * touch + 1e-12
        assert bool(((dg - t("grad_grids")).abs() <= bound).all()), c
        rg = t("grad_rgb")
        rms = float(rg.pow(2).mean().sqrt()) + 1e-30
        ok = (dc - rg).abs() <= 1e-4 * (rg.abs() + rms)
        Lz = grids.shape[2]
        w = (BO.GRAY[0] * rgb[..., 0] + BO.GRAY[1] * rgb[..., 1] + BO.GRAY[2] * rgb[..., 2]) * (Lz - 1)
        near = (w - w.round()).abs() <= 8 * U * (Lz - 1)
        shift = w.round() - w
        for s in (1e-9, -1e-9):
            a = BO.slice_grads(grids, xy, rgb, idx, dout, w_shift=shift + s)[2]
            ok |= near.unsqueeze(-1) & ((a - rg).abs() <= 1e-4 * (rg.abs() + rms))
        assert bool(ok.all()), f"{c}: {int((~ok).sum())} colour-gradient elements"
    for n in (1, 3):
        x = torch.from_numpy(z[f"tv{n}_x"]).double()
        val, g = BO.tv_grads(x)
        assert abs(float(val) - float(z[f"tv{n}_value"])) <= 1e-5 * float(val)
        ref = torch.from_numpy(z[f"tv{n}_grad"]).double()
        assert bool(((g - ref).abs() <= 1e-5 * (ref.abs() + float(ref.pow(2).mean().sqrt()))).all())


def test_ops_refuse_cpu_tensors():
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.bilagrid_slice(torch.zeros(1, 12, 2, 2, 2), torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 2, 3), torch.zeros(1, 1, dtype=torch.long))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.bilagrid_tv(torch.zeros(1, 12, 2, 2, 2))

"""The bilateral-grid kernels (csrc/bilagrid.hip, include/gspl_hip.h section 14) and `gspl_amd.bilagrid` on the GPU against the fp64
oracle of tests/bilagrid_oracle.py: forward and both gradients in both image layouts, batches with distinct and shared grids, small,
odd and 1080p images, incoherent xy; bit-identical backward whatever the buffers held, guard bands around every buffer, no host
synchronisation, out-of-range indices, the TV loss, and short training runs through the HIP renderer."""
import ctypes
import math

import numpy as np
import pytest
import torch

import gspl_amd  # noqa: F401
from gspl_amd import _lib as L
from gspl_amd import ops, synthetic
from gspl_amd import bilagrid as BG

import bilagrid_oracle as BO
from fakes import FakeCamera, FakeGaussianModel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24


def _grids(n, gx, gy, gw, seed, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    return (BO.identity_grids(n, gx, gy, gw, torch.float32) + scale * torch.randn(n, 12, gw, gy, gx, generator=g)).to(DEV)


def _images(B, H, W, seed, lo=-0.25, hi=1.25, extremes=True):
    g = torch.Generator().manual_seed(seed)
    rgb = lo + (hi - lo) * torch.rand(B, H, W, 3, generator=g)
    if extremes and H * W >= 4:
        rgb.view(B, -1, 3)[:, 0] = 0.0                   # gray exactly 0 and 1 (and beyond)
        rgb.view(B, -1, 3)[:, 1] = 1.0
        rgb.view(B, -1, 3)[:, 2] = 2.0
    return rgb.to(DEV)


def _in_layout(rgb, layout):
    if layout == "hwc":
        return rgb.contiguous()
    return rgb.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)       # a channels-last view of planar images


def _check(grids, xy, rgb, idx_list, grid_idx, seed, layout, tag):
    """HIP forward + backward against the oracle at the issue's bounds."""
    B, H, W, _ = rgb.shape
    Lz = grids.shape[2]
    dout = torch.randn(B, H, W, 3, generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
    g = grids.clone().requires_grad_(True)
    c = _in_layout(rgb, layout).requires_grad_(True)
    out = ops.bilagrid_slice(g, xy, c, grid_idx)
    assert out.stride() == c.stride(), f"{tag}: output layout {out.stride()} differs from the input's {c.stride()}"
    out.backward(dout)
    ref, dg, dc, terms = BO.slice_grads(grids, xy, rgb, idx_list, dout)
    o = out.detach().double()
    err = (o - ref).abs() / (1 + ref.abs())
    assert float(err.max()) <= 1e-6, f"{tag}: forward worst {float(err.max()):.3e}"
    # each grid-gradient element within 1e-5 sum|terms|, plus what rounding the fp32 coordinates can move a tent weight by (a few
    # ulps of the grid size) over the pixels whose cell touches the element: a pixel whose fp32 guidance lands exactly on a level,
    # where the fp64 one lies a hair below it, gives the level under it a weight of ~1e-16 in the oracle and 0 on the GPU
    gg = g.grad.double()
    touch = BO.touch_terms(grids, xy, rgb, idx_list, dout)
    bound = 1e-5 * terms + 16 * U * max(grids.shape[2:]) * touch + 1e-30
    bad = (gg - dg).abs() > bound
    assert not bool(bad.any()), f"{tag}: {int(bad.sum())} grid-gradient elements beyond the bound (worst " \
        f"{float(((gg - dg).abs() / bound).max()):.3e} of it)"
    # colour gradient: pixels whose w lies within 4 ulp (L - 1) of an integer or a bound may take either one-sided difference
    gc = c.grad.double()
    rms = float(dc.pow(2).mean().sqrt()) + 1e-30
    tol = 1e-5 * (dc.abs() + rms)
    ok = (gc - dc).abs() <= tol
    w = (BO.GRAY[0] * rgb[..., 0].double() + BO.GRAY[1] * rgb[..., 1].double() + BO.GRAY[2] * rgb[..., 2].double()) * (Lz - 1)
    near = ((w - w.round()).abs() <= 4 * U * (Lz - 1)) & (w > -4 * U * (Lz - 1)) & (w < (Lz - 1) * (1 + 4 * U))
    if bool(near.any()):
        shift = (w.round() - w).unsqueeze(-1).expand(B, H, W, 1)[..., 0]
        alts = [BO.slice_grads(grids, xy, rgb, idx_list, dout, w_shift=shift + s)[2] for s in (1e-9, -1e-9)]
        alt_ok = torch.zeros_like(ok)
        for a in alts:
            alt_ok |= (gc - a).abs() <= 1e-5 * (a.abs() + rms)
        ok = ok | (near.unsqueeze(-1) & alt_ok)
    assert bool(ok.all()), f"{tag}: {int((~ok).sum())} colour-gradient elements beyond 1e-5 (|ref| + rms)"
    return out, g.grad, c.grad


CASES = [  # (B, H, W, (gx, gy, gw), idx per image, grid_idx shape)
    (1, 1, 1, (16, 16, 8), [0], "one"),
    (1, 1, 17, (8, 8, 4), [2], "one"),
    (2, 13, 1, (16, 16, 8), [1, 0], "rows"),
    (2, 37, 23, (8, 8, 4), [2, 2], "one"),
    (2, 37, 23, (16, 16, 8), [0, 2], "rows"),
    (1, 200, 300, (16, 16, 8), [1], "one"),
]


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_slice_against_the_oracle(case, layout):
    B, H, W, (gx, gy, gw), idx, shape = CASES[case]
    grids = _grids(3, gx, gy, gw, seed=case)
    rgb = _images(B, H, W, seed=10 + case)
    xy = BO.meshgrid_xy(H, W, DEV)
    grid_idx = torch.tensor([[idx[0]]], device=DEV) if shape == "one" else torch.tensor(idx, device=DEV).reshape(B, 1)
    _check(grids, xy, rgb, idx if shape == "rows" else [idx[0]] * B, grid_idx, 100 + case, layout, f"case {case} {layout}")


def test_slice_1080p_both_layouts():
    H, W = 1080, 1920
    grids = _grids(4, 16, 16, 8, seed=5, scale=0.2)
    rgb = _images(1, H, W, seed=6, lo=0.0, hi=1.0)
    xy = BO.meshgrid_xy(H, W, DEV)
    gi = torch.tensor([[3]], device=DEV)
    for layout in ("chw", "hwc"):
        _check(grids, xy, rgb, [3], gi, 7, layout, f"1080p {layout}")


def test_slice_incoherent_xy():
    """Random xy: every block touches the whole grid (the window is walked tile by tile); still the exact sum."""
    B, H, W = 2, 150, 130
    grids = _grids(2, 16, 16, 8, seed=8)
    rgb = _images(B, H, W, seed=9)
    xy = torch.rand(B, H, W, 2, generator=torch.Generator().manual_seed(10)).to(DEV)
    _check(grids, xy, rgb, [1, 0], torch.tensor([[1], [0]], device=DEV), 11, "chw", "random xy")
    _check(grids, xy[:1], rgb[:1], [1], torch.tensor([[1]], device=DEV), 12, "hwc", "random xy, one image")


def _backward_bits(grids, xy, rgb, grid_idx, dout):
    g = grids.clone().requires_grad_(True)
    c = rgb.clone().requires_grad_(True)
    ops.bilagrid_slice(g, xy, c, grid_idx).backward(dout)
    t = ops.bilagrid_tv(g.detach().clone().requires_grad_(True))
    return g.grad.clone(), c.grad.clone(), t.detach().clone()


def _poison_cache(byte):
    """Fill a large block and free it: the caching allocator hands its memory out again to the next allocations."""
    x = torch.empty((512 << 20,), dtype=torch.uint8, device=DEV)
    x.fill_(byte)
    torch.cuda.synchronize()
    del x


def test_backward_is_bit_identical_whatever_the_buffers_held():
    H, W = 540, 960
    grids = _grids(3, 16, 16, 8, seed=20)
    rgb = _images(2, H, W, seed=21)
    xy = BO.meshgrid_xy(H, W, DEV)
    dout = torch.randn(2, H, W, 3, generator=torch.Generator().manual_seed(22)).to(DEV)
    gi = torch.tensor([[2], [0]], device=DEV)
    first = _backward_bits(grids, xy, rgb, gi, dout)
    runs = [_backward_bits(grids, xy, rgb, gi, dout) for _ in range(2)]
    for byte in (0xFF, 0x00):
        _poison_cache(byte)
        runs.append(_backward_bits(grids, xy, rgb, gi, dout))
    for r in runs:
        for a, b in zip(first, r):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert bool(first[0][1].eq(0).all()), "the grid no image selects must get a zero gradient"


GUARD = 4096


def _guarded(nbytes):
    outer = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return outer, outer[GUARD:GUARD + nbytes]


def _intact(outer, nbytes, what):
    assert bool((outer[:GUARD] == 0xA5).all()) and bool((outer[GUARD + nbytes:] == 0xA5).all()), f"a write outside {what}"


@pytest.mark.parametrize("random_xy", [False, True])
def test_no_write_outside_the_buffers(random_xy):
    B, H, W, N, Lz, GH, GW = 2, 97, 131, 3, 8, 16, 16
    grids = _grids(N, GW, GH, Lz, seed=30)
    rgb = _images(B, H, W, seed=31).contiguous()
    xy = (torch.rand(B, H, W, 2, generator=torch.Generator().manual_seed(32)).to(DEV) if random_xy
          else BO.meshgrid_xy(H, W, DEV).expand(B, H, W, 2).contiguous())
    dout = torch.randn(B, H, W, 3, generator=torch.Generator().manual_seed(33)).to(DEV)
    idx = torch.tensor([1, 7], dtype=torch.int32, device=DEV)            # image 1: out of range
    ws_bytes = int(L.lib().gspl_bilagrid_workspace_bytes(Lz, GH, GW, B, H, W))
    sizes = {"out": B * H * W * 12, "grad_grids": grids.numel() * 4, "grad_rgb": B * H * W * 12, "workspace": ws_bytes}
    bufs = {k: _guarded(n) for k, n in sizes.items()}
    p = lambda k: ctypes.c_void_p(bufs[k][1].data_ptr())
    L.call("gspl_bilagrid_slice_fwd", N, Lz, GH, GW, B, H, W, L.ptr(grids), L.ptr(xy), H * W * 2, L.ptr(rgb), L.GSPL_LAYOUT_HWC,
           L.ptr(idx), 1, p("out"), L.stream())
    L.call("gspl_bilagrid_slice_bwd", N, Lz, GH, GW, B, H, W, L.ptr(grids), L.ptr(xy), H * W * 2, L.ptr(rgb), L.GSPL_LAYOUT_HWC,
           L.ptr(idx), 1, L.ptr(dout), L.GSPL_LAYOUT_HWC, p("grad_grids"), p("grad_rgb"), L.GSPL_LAYOUT_HWC, p("workspace"), ws_bytes,
           L.stream())
    torch.cuda.synchronize()
    for k, n in sizes.items():
        _intact(bufs[k][0], n, k)
    out = bufs["out"][1].view(torch.float32).reshape(B, H, W, 3)
    assert bool(out[1].isnan().all()) and bool(out[0].isfinite().all())


def test_out_of_range_index_gives_nan_rows_and_no_gradient():
    H, W = 33, 45
    grids = _grids(3, 16, 16, 8, seed=40)
    rgb = _images(2, H, W, seed=41)
    xy = BO.meshgrid_xy(H, W, DEV)
    dout = torch.randn(2, H, W, 3, generator=torch.Generator().manual_seed(42)).to(DEV)
    for bad in (3, -1, 1 << 20):
        g = grids.clone().requires_grad_(True)
        c = rgb.clone().requires_grad_(True)
        out = ops.bilagrid_slice(g, xy, c, torch.tensor([[1], [bad]], device=DEV))
        out.backward(dout)
        torch.cuda.synchronize()
        assert bool(out[1].isnan().all()) and bool(out[0].isfinite().all())
        _, dg, _, _ = BO.slice_grads(grids, xy, rgb[:1], [1], dout[:1])
        assert torch.allclose(g.grad.double(), dg, rtol=1e-4, atol=1e-5), "the out-of-range image must add nothing"
        assert bool(c.grad[1].isnan().all()) and bool(c.grad[0].isfinite().all())
    out = ops.bilagrid_slice(grids, xy, rgb, torch.tensor([[9]], device=DEV))
    assert bool(out.isnan().all())


def test_no_host_synchronisation():
    H, W = 120, 160
    bg = BG.BilateralGrid(4).to(DEV)
    rgb = _images(1, H, W, seed=50, lo=0, hi=1).permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1).requires_grad_(True)
    xy = BO.meshgrid_xy(H, W, DEV)
    gi = torch.tensor([[2]], device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = BG.slice(bg, xy, rgb, gi)["rgb"]
        loss = out.square().mean() + 10 * BG.total_variation_loss(bg.grids)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert bg.grids.grad is not None and rgb.grad is not None


@pytest.mark.parametrize("n,size", [(1, (16, 16, 8)), (3, (16, 16, 8)), (300, (16, 16, 8)), (3, (5, 12, 3)), (2, (7, 1, 4))])
def test_tv_against_the_oracle(n, size):
    gx, gy, gw = size
    x = _grids(n, gx, gy, gw, seed=60 + n, scale=0.5)
    xg = x.clone().requires_grad_(True)
    t = ops.bilagrid_tv(xg)
    (2.5 * t).backward()
    ref, gref = BO.tv_grads(x)
    assert abs(float(t) - float(ref)) <= 1e-5 * abs(float(ref)) + 1e-12
    g = xg.grad.double()
    rms = float((2.5 * gref).pow(2).mean().sqrt())
    assert bool(((g - 2.5 * gref).abs() <= 1e-5 * ((2.5 * gref).abs() + rms)).all())


def test_module_contract_on_the_gpu():
    bg = BG.BilateralGrid(3, grid_X=8, grid_Y=6, grid_W=4).to(DEV)
    assert tuple(bg.grids.shape) == (3, 12, 4, 6, 8) and set(bg.state_dict()) == {"grids", "rgb2gray_weight"}
    rgb = _images(1, 9, 11, seed=70, lo=0, hi=1)
    out = BG.slice(bg, BO.meshgrid_xy(9, 11, DEV), rgb, torch.tensor([[1]], device=DEV))["rgb"]
    assert torch.allclose(out, rgb, atol=1e-6), "the identity grid must give the colours back"
    assert float(bg.tv_loss()) == 0.0
    with pytest.raises(NotImplementedError):
        BG.slice(bg, torch.zeros(5, 2, device=DEV), torch.zeros(5, 3, device=DEV), torch.zeros(5, 1, dtype=torch.long, device=DEV))
    with pytest.raises(ValueError, match="xy"):
        ops.bilagrid_slice(bg.grids, BO.meshgrid_xy(9, 11, DEV).requires_grad_(True), rgb, torch.tensor([[0]], device=DEV))
    with pytest.raises(ValueError):
        BG.BilateralGrid(1, grid_W=29)


def _target_grids(n, gx=16, gy=16, gw=8):
    """A known smooth per-view grid: gain and offset varying slowly over (x, y, guidance)."""
    z, y, x = torch.meshgrid(torch.linspace(0, 1, gw), torch.linspace(0, 1, gy), torch.linspace(0, 1, gx), indexing="ij")
    out = BO.identity_grids(n, gx, gy, gw, torch.float64).clone()
    for v in range(n):
        for i in range(3):
            out[v, 4 * i + i] += 0.08 * torch.sin(2.0 * x + 1.3 * y + v + i) * (0.5 + 0.5 * z)
            out[v, 4 * i + 3] += 0.03 * torch.cos(1.7 * y - 0.9 * x + 0.5 * v - i)
    return out


def _scene_views(W=192, H=128, n_views=6):
    from gspl_amd.renderers import HipVanillaRenderer
    means, scales, quats, opac, shs = synthetic.scene(20000, seed=11)
    model = FakeGaussianModel(*[t.to(DEV) for t in (means, scales * 3, quats, opac, shs)])
    cams = [FakeCamera(c, DEV) for c in synthetic.camera_set(W, H, 160.0, count=n_views)]
    return HipVanillaRenderer(), model, cams


def test_training_recovers_a_known_grid_and_passes_gradients_to_the_gaussians():
    """Targets: the HIP renders of 6 views through the oracle's slice with a known smooth grid per view.  Only the grids train, 300
    steps of the processor's Adam (lr 2e-3, eps 1e-15) with TV weight 10, all six views per step (B = 6).  Criterion, fixed before the
    first run: the final L1 is at most 0.25 x the initial.  Then, with the Gaussians trainable too, their gradients are finite and
    not all zero."""
    renderer, model, cams = _scene_views()
    bg = torch.zeros(3, device=DEV)
    n = len(cams)
    with torch.no_grad():
        renders = torch.stack([renderer(c, model, bg)["render"] for c in cams])            # [6, 3, H, W]
    H, W = renders.shape[-2:]
    xy = BO.meshgrid_xy(H, W, DEV)
    rgb = renders.permute(0, 2, 3, 1)                                                       # the reference's channels-last view
    target = BO.slice(_target_grids(n).to(DEV), xy.double(), rgb.double(), list(range(n))).float()
    grid = BG.BilateralGrid(n).to(DEV)
    opt = torch.optim.Adam(grid.parameters(), lr=2e-3, eps=1e-15)
    gi = torch.arange(n, device=DEV).reshape(n, 1)

    def l1():
        with torch.no_grad():
            return float((BG.slice(grid, xy, rgb, gi)["rgb"] - target).abs().mean())
    first = l1()
    for _ in range(300):
        out = BG.slice(grid, xy, rgb, gi)["rgb"]
        loss = (out - target).abs().mean() + 10 * grid.tv_loss()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    last = l1()
    assert first > 1e-3 and last <= 0.25 * first, f"L1 {first:.5f} -> {last:.5f}"
    # the Gaussians trainable too: gradients flow through the slice into the renderer
    for p in model.parameters():
        p.grad = None
    for step in range(3):
        cam = cams[step]
        img = renderer(cam, model, bg)["render"]
        out = BG.slice(grid, xy, img.permute(1, 2, 0).unsqueeze(0), torch.tensor([[step]], device=DEV))["rgb"].squeeze(0).permute(2, 0, 1)
        assert out.is_contiguous(), "the processor's permute back must give a contiguous CHW image"
        ((out - target[step].permute(2, 0, 1)).abs().mean() + 10 * grid.tv_loss()).backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(bool(g.isfinite().all()) for g in grads) and any(bool(g.ne(0).any()) for g in grads)
    assert bool(grid.grids.grad.isfinite().all())

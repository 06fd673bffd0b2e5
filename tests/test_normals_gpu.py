"""The normal-map kernels (csrc/normals.hip, include/gspl_hip.h section 15) and `ops.depth_to_normal` / `ops.surfel_maps` /
`ops.surface_reg` on the GPU against the fp64 oracle of tests/normals_oracle.py.

Inputs (seeded, tests/normals_oracle.py): depth = 3 + 0.01 x + 0.02 y + 0.3 sin(x / 5) cos(y / 7) + 0.05 rand with a +2 step over the
lower-right quadrant; A = R(random unit quaternion) K^-1, principal point at the centre, f = 170 (1600 at 1080p).

Forward, every interior element: |n - n_ref| <= 4 U + KAPPA U S / |c|, U = 2^-24, S = (|q(y+1,x)| + |q(y-1,x)|) |dy| + (|q(y,x+1)| +
|q(y,x-1)|) |dx| and |c| from the oracle: 4 U for the normalisation, S / |c| for what rounding the four points moves the cross product
by.  KAPPA: the reference's own fp32 torch arithmetic (this file's `torch32_kappa`, the oracle's formulation run in fp32 on the CPU) needs
kappa = 1.10 on exactly these inputs (re-measured on a CPU: 0.04, 0.37, 0.45, 0.77, 1.10 from 3 x 3 to 1080 x 1920; up to 1.00 with
normalize_rays at the three shapes tested with it; 1.23 was measured with other seeds when the check was specified); the kernel gets
4 x that, rounded up to a power of two, for another operation order and FMA contraction: KAPPA = 8 (4.4 and 4.9 round up alike).

Backward, upstream gradient randn: E = max |g - g_ref| / (|g_ref| + rms) over the case, required E <= max(1e-4, 4 E_torch32) with
E_torch32 computed here, on the CPU, from fp32 autograd of the same formulation (measured: <= 4.3e-5 up to 128 x 176, 1.4e-3 at 1080p
with f = 1600, where the cross products are ~1e-6 of the points: hence the bound relative to it).

Where the depth map is exactly 0 over a block the forward is exactly 0; the generic backward is only required to be finite there: below
eps the normalisation keeps torch's constant denominator, so gradients next to such a block carry a 1 / 1e-12 scale.

`ops.surfel_maps`: surf_depth within 4 U |ref| (the fp32 quotient, rho and the result are the kernel's three roundings); rend_normal
within 4 U sum_j |R_ij| |v_j| (a three-term dot product: relative to its terms, since the sum itself may cancel); surf_normal by the
forward bound times alpha (plus U |ref| for that product), all gradients by the backward bound, per plane of v_allmap.  Plane 6 and the
pixels where nan_to_num replaced the value are exactly 0 (torch leaves NaN in planes 0 and 1 at alpha = 0; the oracle routes around it).

`ops.surface_reg`: |out - ref| <= GAMMA mean|terms|, the terms of out[0] being 1 and the three products a_c b_c of every pixel (the sum
1 - a.b may cancel), those of out[1] the values of dist.  GAMMA = U x (the longest serial chain, 64, plus the tree depth, 9, at both
levels of the sum — the constants kRegChain and kRegTree of csrc/normals.hip — plus 6 for the roundings of a term and of the final
product with 1 / (H W))."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import gspl_amd  # noqa: F401
from gspl_amd import _lib as L
from gspl_amd import ops

import normals_oracle as NO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
KAPPA = 8.0
REG_CHAIN, REG_TREE = 64, 9                    # kRegChain, kRegTree of csrc/normals.hip
GAMMA = U * (2 * (REG_CHAIN + REG_TREE) + 6)

SHAPES = [(1, 1), (2, 5), (3, 3), (5, 67), (37, 50), (128, 176), (1080, 1920)]


@functools.lru_cache(maxsize=None)
def _inputs(H, W):
    seed = H * 7 + W
    return NO.case_depth(H, W, seed), NO.case_rays(H, W, seed)


def _upstream(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _E(g, ref):
    ref = ref.double()
    rms = float(ref.pow(2).mean().sqrt())
    return float(((g.double() - ref).abs() / (ref.abs() + rms + 1e-300)).max())


@functools.lru_cache(maxsize=None)
def _reference(H, W, normalize_rays):
    """(n_ref [H,W,3], S, |c|, g_ref [H,W], E_torch32, kappa_torch32) of a case: computed once, shared, never modified."""
    depth, A = _inputs(H, W)
    v = _upstream((H, W, 3), H + W)
    if H < 3 or W < 3:                                             # all zeros, and so is the gradient
        return torch.zeros(H, W, 3, dtype=torch.float64), None, None, torch.zeros(H, W, dtype=torch.float64), 0.0, 0.0
    d64 = depth.double().requires_grad_(True)
    n_ref = NO.depth_to_normal(d64, A.double(), normalize_rays)
    g_ref, = torch.autograd.grad(n_ref, d64, v.double())
    d32 = depth.clone().requires_grad_(True)
    n32 = NO.depth_to_normal(d32, A, normalize_rays)
    g32, = torch.autograd.grad(n32, d32, v)
    S, c = NO.forward_bound_terms(depth, A, normalize_rays)
    err = (n32.detach().double() - n_ref.detach())[1:-1, 1:-1].abs().amax(dim=-1)
    kappa32 = float(((err - 4 * U).clamp_min(0) * c / (U * S)).max())
    return n_ref.detach(), S, c, g_ref, _E(g32, g_ref), kappa32


def torch32_kappa(shapes=SHAPES, normalize_rays=False):
    """The kappa the reference's fp32 torch arithmetic needs on this file's inputs (quoted in the docstring)."""
    return {s: _reference(s[0], s[1], normalize_rays)[5] for s in shapes}


def _check_forward(n, n_ref, S, c, tag, weight=None, extra=None):
    """n [H,W,3] against the oracle at 4 U + KAPPA U S / |c| on every interior element; exactly 0 on the border."""
    H, W, _ = n_ref.shape
    n = n.detach().double().cpu()
    border = torch.ones(H, W, dtype=torch.bool)
    if H >= 3 and W >= 3:
        border[1:-1, 1:-1] = False
        bound = 4 * U + KAPPA * U * S / c
        if weight is not None:
            bound = bound * weight[1:-1, 1:-1]
        bound = bound[..., None] + (0 if extra is None else extra[1:-1, 1:-1])
        err = (n - n_ref)[1:-1, 1:-1].abs()
        bound = bound.expand_as(err)
        worst = float((err[bound > 0] / bound[bound > 0]).max())
        print(f"{tag}: forward worst {worst:.3f} of the bound, max error {float(err.max()):.3e}")
        assert bool((err <= bound).all()), f"{tag}: forward {worst:.3f} x the bound"      # (a bound of 0, where alpha is 0, asks for 0)
    assert float(n[border].abs().max()) == 0.0, f"{tag}: the border must be exactly 0"


def _check_backward(g, g_ref, e32, tag):
    e = _E(g.detach().cpu(), g_ref)
    print(f"{tag}: backward E {e:.3e}, E_torch32 {e32:.3e}")
    assert bool(torch.isfinite(g).all()) and e <= max(1e-4, 4 * e32), f"{tag}: backward E {e:.3e} against {max(1e-4, 4 * e32):.3e}"


def _run(H, W, normalize_rays, channels_first):
    depth, A = _inputs(H, W)
    n_ref, S, c, g_ref, e32, k32 = _reference(H, W, normalize_rays)
    v = _upstream((H, W, 3), H + W)
    d = depth.to(DEV).requires_grad_(True)
    n = ops.depth_to_normal(d, A.to(DEV), normalize_rays=normalize_rays, channels_first=channels_first)
    assert n.shape == ((3, H, W) if channels_first else (H, W, 3)) and n.is_contiguous()
    n.backward((v.permute(2, 0, 1) if channels_first else v).to(DEV).contiguous())
    tag = f"{H}x{W} norm={int(normalize_rays)} chw={int(channels_first)}"
    print(f"{tag}: kappa of fp32 torch {k32:.3f}")
    _check_forward(n.permute(1, 2, 0) if channels_first else n, n_ref, S, c, tag)
    _check_backward(d.grad, g_ref, e32, tag)
    if H < 3 or W < 3:
        assert float(n.detach().abs().max()) == 0.0 and float(d.grad.abs().max()) == 0.0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_depth_to_normal_against_the_oracle(shape):
    _run(shape[0], shape[1], False, False)


@pytest.mark.parametrize("shape", [(5, 67), (37, 50), (128, 176)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("normalize_rays,channels_first", [(True, False), (False, True), (True, True)])
def test_depth_to_normal_normalized_rays_and_planar_layout(shape, normalize_rays, channels_first):
    _run(shape[0], shape[1], normalize_rays, channels_first)


def test_zero_depth_block_gives_zero_normals_and_finite_gradients():
    H, W = 37, 50
    depth, A = _inputs(H, W)
    depth = depth.clone()
    depth[10:17, 20:27] = 0.0                                       # 7 x 7, exactly zero
    v = _upstream((H, W, 3), 5).to(DEV)
    d = depth.to(DEV).requires_grad_(True)
    n = ops.depth_to_normal(d, A.to(DEV))
    n.backward(v)
    assert float(n.detach()[11:16, 21:26].abs().max()) == 0.0                # the centres whose four points all lie in the block
    assert bool(torch.isfinite(n).all()) and bool(torch.isfinite(d.grad).all())
    assert float(d.grad[12:15, 22:25].abs().max()) == 0.0           # every centre that reads these has dx = dy = 0
    S, c = NO.forward_bound_terms(depth, A)
    keep = c > 1e-9                                                 # elsewhere the oracle's bounds still hold
    err = (n.detach().double().cpu() - NO.depth_to_normal(depth.double(), A.double()))[1:-1, 1:-1].abs().amax(-1)
    assert bool((err[keep] <= (4 * U + KAPPA * U * S / c)[keep]).all())


def test_gsplat_utils_stand_in_on_the_gpu():
    """`gsplat.utils.depth_to_normal` (pixel centres at +0.5, z_depth and ray-distance forms, a batch of images) at the same bounds."""
    from gspl_amd import compat
    compat.install()
    import gsplat
    if "gspl_amd" not in (gsplat.__doc__ or ""):
        pytest.skip("a real gsplat package is installed")
    from gsplat.utils import depth_to_normal
    H, W = 37, 50
    depth = torch.stack([NO.case_depth(H, W, 40), NO.case_depth(H, W, 41)])
    c2w = torch.eye(4).repeat(2, 1, 1)
    c2w[0, :3, :3], c2w[1, :3, :3] = NO.case_rotation(40).float(), NO.case_rotation(41).float()
    c2w[:, :3, 3] = torch.tensor([[0.3, -1.0, 2.0], [5.0, 0.1, -0.7]])
    K = torch.tensor([[170.0, 0, 24.3], [0, 168.0, 19.1], [0, 0, 1]]).repeat(2, 1, 1)
    v = _upstream((2, H, W, 3), 42)
    for z_depth in (True, False):
        d = depth.to(DEV).requires_grad_(True)
        out = depth_to_normal(d[..., None], c2w.to(DEV), K.to(DEV), z_depth=z_depth)
        assert out.shape == (2, H, W, 3)
        out.backward(v.to(DEV))
        for i in range(2):
            A = NO.gsplat_rays(c2w[i].double(), K[i].double())
            d64 = depth[i].double().requires_grad_(True)
            n_ref = NO.depth_to_normal(d64, A, not z_depth)
            g_ref, = torch.autograd.grad(n_ref, d64, v[i].double())
            d32 = depth[i].clone().requires_grad_(True)
            g32, = torch.autograd.grad(NO.depth_to_normal(d32, NO.gsplat_rays(c2w[i], K[i]), not z_depth), d32, v[i])
            S, c = NO.forward_bound_terms(depth[i], A, not z_depth)
            _check_forward(out[i], n_ref.detach(), S, c, f"gsplat image {i} z_depth={z_depth}")
            _check_backward(d.grad[i], g_ref, _E(g32, g_ref), f"gsplat image {i} z_depth={z_depth}")
        # the half-pixel offset is there: the same call with the principal point moved by 0.5 equals the integer-centre stencil
        A_int = (c2w[0, :3, :3].double() @ torch.tensor([[1 / 170.0, 0, -24.3 / 170.0], [0, 1 / 168.0, -19.1 / 168.0], [0, 0, 1]], dtype=torch.float64))
        shifted = depth_to_normal(depth[0].to(DEV)[..., None], c2w[0].to(DEV), (K[0] + torch.tensor([[0, 0, 0.5], [0, 0, 0.5], [0, 0, 0]])).to(DEV),
                                  z_depth=z_depth)
        S, c = NO.forward_bound_terms(depth[0], A_int, not z_depth)
        _check_forward(shifted, NO.depth_to_normal(depth[0].double(), A_int, not z_depth), S, c, "gsplat, principal point + 0.5")


# ---- the 2DGS maps ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _allmap(H, W):
    """depth | alpha | view normal x3 | median | distortion, with alpha exactly 0 over a block (0 / 0 and x / 0) and 1e-6 over another."""
    g = torch.Generator().manual_seed(H * 3 + W)
    depth, _ = _inputs(H, W)
    alpha = 0.2 + 0.8 * torch.rand(H, W, generator=g)
    alpha[H // 8:H // 8 + 6, W // 8:W // 8 + 7] = 1e-6
    a0 = depth * alpha
    alpha[H // 2:H // 2 + 6, W // 3:W // 3 + 8] = 0.0
    a0[H // 2:H // 2 + 6, W // 3:W // 3 + 4] = 0.0                 # 0 / 0 -> NaN -> 0; the other half stays positive: x / 0 -> +inf -> 0
    median = depth + 0.02 * torch.randn(H, W, generator=g)
    median[H // 2 + 1, W // 3 + 1] = float("nan")
    median[H // 2 + 2, W // 3 + 2] = float("inf")
    normals = torch.randn(3, H, W, generator=g) * alpha
    dist = torch.rand(H, W, generator=g) * 1e-2
    return torch.cat([a0[None], alpha[None], normals, median[None], dist[None]]).contiguous()


@pytest.mark.parametrize("rho", [0.0, 1.0, 0.3])
@pytest.mark.parametrize("shape", [(37, 50), (128, 176)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_surfel_maps_against_the_oracle(shape, rho):
    H, W = shape
    allmap, (_, A) = _allmap(H, W), _inputs(H, W)
    R = NO.case_rotation(H).float()
    ups = [_upstream((3, H, W), 1), _upstream((1, H, W), 2), _upstream((3, H, W), 3)]
    tag = f"surfel_maps {H}x{W} rho={rho}"

    def oracle(dtype):
        a = allmap.clone().to(dtype).requires_grad_(True)
        outs = NO.surfel_maps(a, R.to(dtype), A.to(dtype), rho)
        g, = torch.autograd.grad(outs, a, [u.to(dtype) for u in ups])
        return [o.detach() for o in outs], g
    (rn_ref, sd_ref, sn_ref), g_ref = oracle(torch.float64)
    _, g32 = oracle(torch.float32)

    a = allmap.to(DEV).requires_grad_(True)
    rn, sd, sn = ops.surfel_maps(a, R.to(DEV), A.to(DEV), rho)
    assert rn.shape == (3, H, W) and sd.shape == (1, H, W) and sn.shape == (3, H, W)
    torch.autograd.backward([rn, sd, sn], [u.to(DEV) for u in ups])
    rn, sd, sn, g = rn.detach().double().cpu(), sd.detach().double().cpu(), sn.detach().double().cpu(), a.grad.cpu()

    assert bool(((sd - sd_ref).abs() <= 4 * U * sd_ref.abs()).all()), f"{tag}: surf_depth worst {float(((sd - sd_ref).abs() / sd_ref.abs().clamp_min(1e-30)).max()) / U:.2f} U"
    terms = (R.double().abs() @ allmap[2:5].double().abs().reshape(3, -1)).reshape(3, H, W)
    assert bool(((rn - rn_ref).abs() <= 4 * U * terms).all()), f"{tag}: rend_normal"
    S, c = NO.forward_bound_terms(sd_ref[0], A)
    ok = c > 0                                                      # (inside the alpha = 0 block surf_depth is 0 and so is the normal)
    alpha = allmap[1].double()
    S, c = torch.where(ok, S, torch.zeros_like(S)), torch.where(ok, c, torch.ones_like(c))
    _check_forward(sn.permute(1, 2, 0), sn_ref.permute(1, 2, 0), S, c, tag, weight=alpha, extra=U * sn_ref.permute(1, 2, 0).abs())

    masked01 = ~torch.isfinite(allmap[0] / allmap[1])
    masked5 = ~torch.isfinite(allmap[5])
    assert int(masked01.sum()) >= 48 and int(masked5.sum()) == 2
    assert float(g[6].abs().max()) == 0.0, f"{tag}: plane 6"
    assert float(g[0][masked01].abs().max()) == 0.0 and float(g[1][masked01].abs().max()) == 0.0 and float(g[5][masked5].abs().max()) == 0.0
    assert bool(torch.isfinite(g).all())
    for plane in range(7):
        if float(g_ref[plane].abs().max()) == 0.0:
            assert float(g[plane].abs().max()) == 0.0, f"{tag}: plane {plane} must be 0"
            continue
        _check_backward(g[plane], g_ref[plane], _E(g32[plane], g_ref[plane]), f"{tag} plane {plane}")


def test_surfel_maps_with_absent_upstream_gradients():
    H, W = 37, 50
    allmap, (_, A) = _allmap(H, W), _inputs(H, W)
    R = NO.case_rotation(H).float()
    for which in range(3):
        a = allmap.to(DEV).requires_grad_(True)
        outs = ops.surfel_maps(a, R.to(DEV), A.to(DEV), 0.3)
        up = _upstream(tuple(outs[which].shape), which)
        outs[which].backward(up.to(DEV))
        a64 = allmap.double().requires_grad_(True)
        g_ref, = torch.autograd.grad(NO.surfel_maps(a64, R.double(), A.double(), 0.3)[which], a64, up.double())
        used = [p for p in range(7) if float(g_ref[p].abs().max()) > 0]
        assert used == [[2, 3, 4], [0, 1, 5], [0, 1, 5]][which]
        for p in range(7):
            if p in used:
                assert _E(a.grad[p].cpu(), g_ref[p]) <= 1e-3
            else:
                assert float(a.grad[p].abs().max()) == 0.0


# ---- the regulariser sums --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_dist", [True, False])
@pytest.mark.parametrize("shape", [(1, 1), (37, 50), (128, 176), (129, 127), (1080, 1920)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_surface_reg_against_the_oracle(shape, with_dist):
    H, W = shape
    g = torch.Generator().manual_seed(H + W)
    a, b, dist = torch.randn(3, H, W, generator=g), torch.randn(3, H, W, generator=g), torch.rand(1, H, W, generator=g)
    assert L.lib().gspl_surface_reg_partials(H * W) == -(-H * W // (256 * REG_CHAIN))
    leaves = [t.to(DEV).requires_grad_(True) for t in (a, b, dist)]
    out = ops.surface_reg(leaves[0], leaves[1], leaves[2] if with_dist else None)
    assert out.shape == (2,)
    w = torch.tensor([1.75, -0.625], device=DEV)              # (exact in fp32)
    (out * w).sum().backward()
    ref = NO.surface_reg(a.double(), b.double(), dist.double()[0] if with_dist else None)
    scale0 = float((1 + (a.double() * b.double()).abs().sum(0)).mean())
    scale1 = float(dist.double().abs().mean())
    o = out.detach().double().cpu()
    print(f"surface_reg {H}x{W}: errors {abs(float(o[0] - ref[0])) / scale0 / U:.2f} U, {abs(float(o[1] - ref[1])) / scale1 / U:.2f} U of the terms; GAMMA = {GAMMA / U:.0f} U")
    assert abs(float(o[0] - ref[0])) <= GAMMA * scale0
    if with_dist:
        assert abs(float(o[1] - ref[1])) <= GAMMA * scale1
        assert bool(((leaves[2].grad.double().cpu() - (-0.625) / (H * W)).abs() <= 4 * U * 0.625 / (H * W)).all())
    else:
        assert float(o[1]) == 0.0 and leaves[2].grad is None
    for got, other in ((leaves[0].grad, b), (leaves[1].grad, a)):
        want = -1.75 * other.double() / (H * W)
        assert bool(((got.double().cpu() - want).abs() <= 4 * U * want.abs()).all())


# ---- robustness ------------------------------------------------------------------------------------------------------------------------
def _poison_cache(byte):
    """Fill a large block and free it: the caching allocator hands its memory out again to the next allocations."""
    x = torch.empty((512 << 20,), dtype=torch.uint8, device=DEV)
    x.fill_(byte)
    torch.cuda.synchronize()
    del x


def _all_bits(H, W):
    depth, A = _inputs(H, W)
    allmap = _allmap(H, W).to(DEV)
    A, R = A.to(DEV), NO.case_rotation(1).float().to(DEV)
    d = depth.to(DEV).requires_grad_(True)
    n = ops.depth_to_normal(d, A, normalize_rays=True)
    n.backward(_upstream((H, W, 3), 1).to(DEV))
    a = allmap.clone().requires_grad_(True)
    rn, sd, sn = ops.surfel_maps(a, R, A, 0.3)
    reg = ops.surface_reg(rn, sn, a[6])
    (reg[0] + 100 * reg[1] + sd.mean()).backward()
    return [t.detach().clone() for t in (n, d.grad, rn, sd, sn, reg, a.grad)]


def test_results_are_bit_identical_whatever_the_buffers_held():
    H, W = 270, 480
    first = _all_bits(H, W)
    runs = [_all_bits(H, W)]
    for byte in (0xFF, 0x00):
        _poison_cache(byte)
        runs.append(_all_bits(H, W))
    for r in runs:
        for x, y in zip(first, r):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


GUARD = 4096


def _guarded(nbytes):
    outer = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return outer, outer[GUARD:GUARD + nbytes]


@pytest.mark.parametrize("shape", [(37, 50), (3, 3), (1, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_no_write_outside_the_buffers(shape):
    H, W = shape
    P = H * W
    g = torch.Generator().manual_seed(9)
    depth = (3 + torch.rand(H, W, generator=g)).to(DEV)
    A, R = NO.case_rays(H, W, 1).to(DEV), NO.case_rotation(1).float().to(DEV)
    allmap = (0.1 + torch.rand(7, H, W, generator=g)).to(DEV)
    v3, v1, go = torch.randn(3, H, W, generator=g).to(DEV), torch.randn(1, H, W, generator=g).to(DEV), torch.tensor([1.0, 2.0], device=DEV)
    n_part = L.lib().gspl_surface_reg_partials(P)
    sizes = {"normal": 12 * P, "v_depth": 4 * P, "rend_normal": 12 * P, "surf_depth": 4 * P, "surf_normal": 12 * P, "v_allmap": 28 * P,
             "partials": 8 * n_part, "out": 8, "v_a": 12 * P, "v_b": 12 * P, "v_dist": 4 * P}
    bufs = {k: _guarded(n) for k, n in sizes.items()}
    p = lambda k: ctypes.c_void_p(bufs[k][1].data_ptr())
    for layout in (L.GSPL_LAYOUT_HWC, L.GSPL_LAYOUT_CHW):
        for norm in (0, 1):
            L.call("gspl_depth_normal_fwd", H, W, L.ptr(depth), L.ptr(A), norm, layout, p("normal"), L.stream())
            L.call("gspl_depth_normal_bwd", H, W, L.ptr(depth), L.ptr(A), norm, L.ptr(v3), layout, p("v_depth"), L.stream())
    L.call("gspl_surfel_maps_fwd", H, W, L.ptr(allmap), L.ptr(R), L.ptr(A), 0.3, p("rend_normal"), p("surf_depth"), p("surf_normal"), L.stream())
    L.call("gspl_surfel_maps_bwd", H, W, L.ptr(allmap), L.ptr(R), L.ptr(A), 0.3, L.ptr(v3), L.ptr(v1), L.ptr(v3), p("v_allmap"), L.stream())
    L.call("gspl_surface_reg_fwd", H, W, L.ptr(v3), L.ptr(allmap), L.ptr(depth), p("partials"), p("out"), L.stream())
    L.call("gspl_surface_reg_bwd", H, W, L.ptr(v3), L.ptr(allmap), L.ptr(go), p("v_a"), p("v_b"), p("v_dist"), L.stream())
    torch.cuda.synchronize()
    for k, n in sizes.items():
        outer = bufs[k][0]
        assert bool((outer[:GUARD] == 0xA5).all()) and bool((outer[GUARD + n:] == 0xA5).all()), f"a write outside {k}"
        assert not bool((bufs[k][1].view(torch.int32) == -1515870811).all()), f"{k} was not written"      # 0xA5A5A5A5


def test_bad_arguments_are_refused():
    H, W = 5, 6
    x = torch.ones(7, H, W, device=DEV)
    with pytest.raises(RuntimeError, match="layout"):
        L.call("gspl_depth_normal_fwd", H, W, L.ptr(x), L.ptr(x), 0, 7, L.ptr(x), L.stream())
    with pytest.raises(RuntimeError, match="NULL"):
        L.call("gspl_surfel_maps_fwd", H, W, L.ptr(x), None, L.ptr(x), 0.0, L.ptr(x), L.ptr(x), L.ptr(x), L.stream())
    with pytest.raises(RuntimeError, match="H W"):
        L.call("gspl_surface_reg_fwd", 0, W, L.ptr(x), L.ptr(x), None, L.ptr(x), L.ptr(x), L.stream())
    with pytest.raises(ValueError):
        ops.surfel_maps(x[:6], torch.eye(3, device=DEV), torch.eye(3, device=DEV), 0.0)
    with pytest.raises(ValueError):
        ops.surface_reg(x[:3], x[:3], x[0, :4])
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.depth_to_normal(x[0], torch.eye(3))
    assert ops.depth_to_normal(torch.ones(0, 4, device=DEV), torch.eye(3, device=DEV)).shape == (0, 4, 3)


def test_no_host_synchronisation():
    depth, A = _inputs(128, 176)
    allmap = _allmap(128, 176).to(DEV).requires_grad_(True)
    A, R = A.to(DEV), NO.case_rotation(2).float().to(DEV)
    d = depth.to(DEV).requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        n = ops.depth_to_normal(d, A, channels_first=True)
        rn, sd, sn = ops.surfel_maps(allmap, R, A, 0.3)
        reg = ops.surface_reg(rn, sn, allmap[6:7])
        loss = 0.05 * reg[0] + 100 * reg[1] + ops.surface_reg(n, rn)[0] + sd.mean()
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(allmap.grad).all()) and bool(torch.isfinite(d.grad).all())


# ---- the plugin ------------------------------------------------------------------------------------------------------------------------
def test_plugin_with_fused_maps_has_the_same_contract():
    from fakes import FakeCamera, FakeGaussianModel
    from gspl_amd.renderers import HipVanilla2DGSRenderer
    from test_surfel_gpu import _special_scene
    params, cam = _special_scene(seed=6)
    means, scales, quats, opac, shs = params
    scales3 = torch.cat([scales, torch.full((scales.shape[0], 1), 1e-3)], dim=1)
    bg = torch.zeros(3, device=DEV)
    outs, grads = {}, {}
    for fused in (False, True):
        model = FakeGaussianModel(*[t.to(DEV) for t in (means, scales3, quats, opac, shs)])
        fcam = FakeCamera(cam, DEV)
        out = HipVanilla2DGSRenderer(depth_ratio=0.3, fused_maps=fused)(fcam, model, bg)
        if fused:
            assert hasattr(fcam, "_gspl_surfel_matrices")
            reg = ops.surface_reg(out["rend_normal"], out["surf_normal"], out["rend_dist"])
            loss = out["render"].mean() + reg[1] + reg[0]
        else:
            loss = out["render"].mean() + out["rend_dist"].mean() + (1 - (out["rend_normal"] * out["surf_normal"]).sum(0)).mean()
        out["viewspace_points"].retain_grad()
        loss.backward()
        assert bool(torch.isfinite(model.means.grad).all()) and float(out["viewspace_points"].grad[:, :2].abs().sum()) > 0
        outs[fused], grads[fused] = out, [p.grad for p in model.parameters() if p.grad is not None]
    assert set(outs[True]) == set(outs[False])
    for k in set(outs[True]) - {"viewspace_points"}:
        x, y = outs[True][k], outs[False][k]
        assert x.shape == y.shape and x.device == y.device == DEV and x.dtype == y.dtype, k
    assert torch.equal(outs[True]["radii"], outs[False]["radii"])
    for k in ("render", "rend_alpha", "view_normal", "rend_dist", "rend_normal", "surf_depth"):      # two renders, a few fp32 roundings apart
        assert torch.allclose(outs[True][k], outs[False][k], rtol=1e-5, atol=1e-6), k
    assert all(bool(torch.isfinite(g).all()) for g in grads[True]) and len(grads[True]) == len(grads[False]) > 0


def test_surfel_training_on_the_fused_maps_and_regulariser():
    """tests/test_surfel_gpu.py's `test_surfel_training_with_normal_and_distortion_losses` with everything after the rasterizer on
    `ops.surfel_maps` + `ops.surface_reg`: the same scene, optimiser, weights, 200 steps and criterion."""
    from fakes import FakeCamera
    from gspl_amd.renderers import HipVanilla2DGSRenderer
    from test_surfel_gpu import _settings, _special_scene
    params, cam = _special_scene(seed=12, n=800)
    target_params, _ = _special_scene(seed=13, n=800)
    bg = torch.tensor([0.0, 0.0, 0.0], device=DEV)
    st = _settings(cam, bg, 1.0, DEV)
    with torch.no_grad():
        m, s, q, o, c = [t.to(DEV).float() for t in target_params]
        target = ops.SurfelGaussianRasterizer(st)(means3D=m, means2D=torch.zeros_like(m), opacities=o, shs=c, scales=s, rotations=q)[0]
    leaves = [t.to(DEV).float().clone().requires_grad_(True) for t in params]
    opt = torch.optim.Adam([{"params": [leaves[0]], "lr": 1e-3}, {"params": leaves[1:3], "lr": 5e-3}, {"params": leaves[3:], "lr": 1e-2}])
    fcam = FakeCamera(cam, DEV)
    losses = []
    for step in range(200):
        m, s, q, o, c = leaves
        screen = torch.zeros_like(m, requires_grad=True)
        color, radii, allmap = ops.SurfelGaussianRasterizer(st)(means3D=m, means2D=screen, opacities=o.clamp(0, 1), shs=c, scales=s.abs(), rotations=q)
        normal_rot, rays = HipVanilla2DGSRenderer.camera_matrices(fcam, allmap)
        rend_normal, _, surf_normal = ops.surfel_maps(allmap, normal_rot, rays, 0.0)
        reg = ops.surface_reg(rend_normal, surf_normal, allmap[6])
        loss = (color - target).abs().mean() + 0.05 * reg[0] + 100.0 * reg[1]
        opt.zero_grad()
        loss.backward()
        for t in leaves:
            assert bool(torch.isfinite(t.grad).all()), step
        opt.step()
        losses.append(float(loss))
    assert all(math.isfinite(v) for v in losses)
    assert np.mean(losses[-20:]) < 0.8 * np.mean(losses[:5]), (losses[:5], losses[-20:])

"""The PVG route on the GPU: csrc/pvg.hip, csrc/envlight.hip, `ops.pvg_motion` / `ops.cubemap_sample` / `ops.envlight_blend` and
`HipPeriodicVibrationGaussianRenderer`, against the fp64 oracle of tests/pvg_oracle.py.

How the kernels' bounds are set.  Every output element and every gradient element is a short sum of products; its error is measured
RELATIVE TO THE SUM OF THE ABSOLUTE VALUES OF ITS TERMS (for a texture gradient: of the absolute contributions to that texel, the
measure a reordered atomic sum obeys).  The bound of a case is 4 x the worst such ratio that the SAME formulation run in float32 torch
on the CPU shows on the same inputs against the same oracle — the test computes that figure and prints it — and never below
8 x 2^-24; the factor 4 allows for the order of the operations, FMA contraction and another libm.  Terms that go through the marginal
are formed with max(marginal, 2^-105): see pvg_oracle.MARGINAL_FLOOR.

fp32-torch figures (the worst ratio over the elements of all cases of a kind; the bound is 4 x the case's own figure, at least
4.77e-07 = 8 x 2^-24) next to the kernels' own worst ratios, as a run on an MI355X printed them: the table at the end of this docstring.

The renderer.  The slices of the single D = 8 pass are required to be BIT-EQUAL to separate `ops.rasterize_gaussians` calls with
D = 3, 3, 1 and 1 on the same lists (the narrow kernels share the alpha code and composite each channel with the same list-order fmaf
chain, whatever D is); the suite's pixel tolerance is not needed.  The gradients of 0.8 L1 + v_reg are compared with fp64 autograd
through the oracle's motion, projection, SH and blend and the C compositing oracle evaluated on the implementation's own lists and
per-splat values (`composite_locked`), pixels that oracle flags as fragile carrying no loss on either side: every element within 1e-4
of |ref| + rms, the suite's gradient tolerance (tests/test_features_gpu.py, tests/test_hip_parity.py).

Measured on an MI355X (fp32-torch figure | kernel | the kernel's worst share of its case's bound):
  motion, N in {1 .. 1000}, shifted and not     means_t 5.08e-06 | 5.12e-06 | 0.28    avg_velocity 2.19e-07 | 2.19e-07 | 0.25
                                                opacity_t 9.02e-06 | 9.02e-06 | 0.25  g_means 0 | 0 (a copy)
                                                g_velocity 3.74e-06 | 3.80e-06 | 0.26 g_t 7.30e-04 | 7.29e-04 | 0.26
                                                g_scale_t 7.86e-07 | 8.11e-07 | 0.32  g_opacities 9.04e-06 | 9.04e-06 | 0.26
    (g_t and the marginal: (t - ts) / scale_t^2 reaches 1e4 before a row underflows, so the float32 rounding of ts and of t - ts
    shows a thousandfold in the exponent; the float32 torch formulation pays exactly the same)
  cubemap forward, R = 1 / 2 / 4 / 16           5.84e-07 | 5.84e-07    9.25e-07 | 9.33e-07    2.08e-06 | 2.07e-06    8.01e-06 | 8.01e-06
  cubemap texture gradient, R = 1 / 2 / 4 / 16  3.42e-08 | 3.58e-08    2.20e-07 | 1.23e-07    1.58e-07 | 1.44e-07    1.10e-05 | 1.10e-05
    (the texel coordinate carries R x 2^-24 of absolute error into a weight, whatever the weight's size: the figures grow with R)
  blend directions (18 cases)                   1.70e-07 | 1.98e-07 | 0.29
  blend forward, R = 2 / 16 (36 cases each)     5.61e-07 | 5.61e-07 | 0.25    3.11e-06 | 3.10e-06 | 0.27
  blend g_alpha, R = 2 / 16                     5.15e-07 | 5.67e-07 | 0.27    4.37e-06 | 4.37e-06 | 0.27
  blend texture gradient, R = 2 / 16            9.06e-06 | 8.95e-06 | 0.27    6.05e-05 | 6.05e-05 | 0.25
The kernels evaluate the taps in the formulation's own order of operations (R a power of two makes the contracted multiply-adds exact),
so most figures coincide.  Renderer: the four map slices were bit-equal to the separate D = 3, 3, 1, 1 passes; no pixel of the 48x64
frames was fragile; every gradient element of means, velocity, t, scale_t, opacities and base passed at 1e-4.
"""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import gspl_amd  # noqa: F401
from gspl_amd import _lib as L
from gspl_amd import ops
from oracle import gsplat_oracle as O

import pvg_oracle as PO
from fakes import FakeCamera
from hip_helpers import assert_close_scaled

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
CYCLE, DECAY, OFFSET, TIME, SHIFT = 0.2, 1.0, -0.5, 0.62, 0.0137


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def _carved(shape, fill=0xFF):
    """A float32 tensor of `shape` inside a guard-banded byte buffer -> (outer bytes, inner tensor, bytes)."""
    nbytes = 4 * int(np.prod(shape))
    outer = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    inner = outer[GUARD:GUARD + nbytes]
    inner.fill_(fill)
    return outer, inner.view(torch.float32).view(shape), nbytes


def _guards_intact(bufs):
    torch.cuda.synchronize()
    for name, (outer, _, nbytes) in bufs.items():
        assert bool((outer[:GUARD] == 0xA5).all()) and bool((outer[GUARD + nbytes:] == 0xA5).all()), f"a write outside {name}"


def _ratio(got, ref, sums):
    """worst |got - ref| / sums over the elements; an element whose terms are all zero must be exact."""
    got, ref, sums = (torch.as_tensor(x).detach().double().cpu().reshape(-1) for x in (got, ref, sums))
    assert got.shape == ref.shape == sums.shape and bool(torch.isfinite(got).all()), "shape mismatch or non-finite values"
    diff = (got - ref).abs()
    zero = sums == 0
    if bool(zero.any()) and float(diff[zero].max()) > 0:
        return math.inf
    return float((diff[~zero] / sums[~zero]).max()) if bool((~zero).any()) else 0.0


def _reorder_bound(texel, weight):
    """Each of two float32 sums of the same n terms, in whatever order, is within (n - 1) 2^-24 of the sum of the absolute terms of
    the exact sum, so the two differ by at most twice that; n: the most taps with a weight that any texel receives."""
    counts = torch.zeros(int(texel.max()) + 1, dtype=torch.int64)
    counts.index_add_(0, texel.reshape(-1), (weight.reshape(-1) != 0).long())
    return max(int(counts.max()) - 1, 1) * 2 * PO.F32_EPS


def _judge(name, gpu, f32, ref, sums):
    """The kernel's worst ratio against 4 x the fp32-torch figure (at least 8 x 2^-24); both printed."""
    figure, worst = _ratio(f32, ref, sums), _ratio(gpu, ref, sums)
    assert math.isfinite(figure), f"{name}: the fp32-torch formulation is off where every term is zero"
    bound = max(4 * figure, PO.MIN_BOUND)
    print(f"{name}: fp32-torch figure {figure:.3e}, bound {bound:.3e}, kernel {worst:.3e}")
    assert worst <= bound, f"{name}: worst ratio {worst:.3e} > bound {bound:.3e} (fp32-torch figure {figure:.3e})"


# ---- 1. the vibration transform -------------------------------------------------------------------------------------------------------
def _motion_direct(inputs, table, upstream):
    """gspl_pvg_motion_fwd / _bwd through the C-ABI into guard-banded buffers."""
    means, velocity, t, scale_t, opac = inputs
    n = means.shape[0]
    bufs = {k: _carved(s) for k, s in (("means_t", (n, 3)), ("avg_velocity", (n, 3)), ("opacity_t", (n, 1)), ("g_means", (n, 3)),
                                       ("g_velocity", (n, 3)), ("g_t", (n, 1)), ("g_scale_t", (n, 1)), ("g_opacities", (n, 1)))}
    b = {k: v[1] for k, v in bufs.items()}
    p = lambda x: L.ptr(x) if n else None
    L.call("gspl_pvg_motion_fwd", n, p(means), p(velocity), p(t), p(scale_t), p(opac), L.ptr(table), p(b["means_t"]), p(b["avg_velocity"]),
           p(b["opacity_t"]), L.stream())
    L.call("gspl_pvg_motion_bwd", n, p(velocity), p(t), p(scale_t), p(opac), L.ptr(table), *[p(g) for g in upstream], p(b["g_means"]),
           p(b["g_velocity"]), p(b["g_t"]), p(b["g_scale_t"]), p(b["g_opacities"]), L.stream())
    _guards_intact(bufs)
    return b


@pytest.mark.parametrize("shifted", [False, True], ids=["unshifted", "shifted"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1000])
def test_motion_forward_and_backward(n, shifted):
    inputs, upstream = PO.motion_case(n)
    shift = SHIFT if shifted else None
    time32 = torch.tensor(TIME, dtype=torch.float32)
    dev_in, dev_up = [x.to(DEV) for x in inputs], [x.to(DEV) for x in upstream]
    table = ops.pvg.motion_table(time32.to(DEV), OFFSET, shift, CYCLE, DECAY, DEV)
    assert table.shape == (6,) and table.dtype == torch.float32
    got = _motion_direct(dev_in, table, dev_up)

    # the op: the same numbers through autograd, the camera's time a device tensor
    leaves = [x.clone().requires_grad_(True) for x in dev_in]
    outs = ops.pvg_motion(*leaves, time32.to(DEV), CYCLE, DECAY, OFFSET, shift)
    assert [tuple(o.shape) for o in outs] == [(n, 3), (n, 3), (n, 1)]
    torch.autograd.backward(outs, dev_up)
    for o, name in zip(outs, ("means_t", "avg_velocity", "opacity_t")):
        assert torch.equal(o.detach(), got[name])
    for leaf, name in zip(leaves, ("g_means", "g_velocity", "g_t", "g_scale_t", "g_opacities")):
        assert leaf.grad.shape == leaf.shape and torch.equal(leaf.grad, got[name])
    if n == 0:
        return

    def formulation(dtype):
        xs = [x.clone().to(dtype).requires_grad_(True) for x in inputs]
        time = time32.to(dtype) if dtype == torch.float32 else float(time32)
        res = PO.motion(*xs, time, OFFSET, shift, CYCLE, DECAY)
        grads = torch.autograd.grad(res, xs, [g.to(dtype) for g in upstream])
        return list(res) + list(grads)

    ref, f32 = formulation(torch.float64), formulation(torch.float32)
    fwd_sums, grad_sums = PO.motion_term_sums(*inputs, float(time32), OFFSET, shift, CYCLE, DECAY, *upstream)
    names = ("means_t", "avg_velocity", "opacity_t", "g_means", "g_velocity", "g_t", "g_scale_t", "g_opacities")
    for name, r, f, s in zip(names, ref, f32, list(fwd_sums) + list(grad_sums)):
        _judge(f"motion n={n} {'shifted' if shifted else 'unshifted'} {name}", got[name], f, r, s)

    # rows whose marginal underflows in float32: exact zeros, and nothing anywhere is NaN or Inf
    # (dead: exp(-110) is far below float32's smallest denormal, 2^-149 = exp(-103.3))
    ts64 = float(time32) + OFFSET - (shift or 0.0)
    dead = (-0.5 * (inputs[2].double() - ts64) ** 2 / inputs[3].double() ** 2 < -110)[:, 0]
    if n >= 257:
        assert 0 < int(dead.sum()) < n
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert not bool(got["opacity_t"].cpu()[dead].any()) and not bool(got["g_opacities"].cpu()[dead].any())
    only_opacity = _motion_direct(dev_in, table, [None, None, dev_up[2]])
    for name in ("g_means", "g_velocity", "g_t", "g_scale_t", "g_opacities"):
        assert bool(torch.isfinite(only_opacity[name]).all())
        assert not bool(only_opacity[name].cpu()[dead].any()), f"{name}: a dead row has a gradient"
    assert bool(only_opacity["g_t"].cpu()[~dead].any()) or n < 63


def test_motion_takes_flat_rows_and_python_time():
    inputs, _ = PO.motion_case(65)
    dev_in = [x.to(DEV) for x in inputs]
    a = ops.pvg_motion(*dev_in, torch.tensor(TIME, device=DEV), CYCLE, DECAY, OFFSET)
    flat = [dev_in[0], dev_in[1]] + [x[:, 0].clone().requires_grad_(True) for x in dev_in[2:]]
    b = ops.pvg_motion(*flat, float(torch.tensor(TIME, dtype=torch.float32)), CYCLE, DECAY, OFFSET)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    b[2].sum().backward()
    assert all(x.grad.shape == (65,) for x in flat[2:])
    # every row keeps its own shape: t [N] next to scale_t [N, 1] and opacities [N]
    mixed = [dev_in[0], dev_in[1], dev_in[2][:, 0].clone().requires_grad_(True), dev_in[3].clone().requires_grad_(True),
             dev_in[4][:, 0].clone().requires_grad_(True)]
    c = ops.pvg_motion(*mixed, torch.tensor(TIME, device=DEV), CYCLE, DECAY, OFFSET)
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    c[2].sum().backward()
    assert [tuple(x.grad.shape) for x in mixed[2:]] == [(65,), (65, 1), (65,)]
    assert all(torch.equal(x.grad.reshape(-1), y.grad.reshape(-1)) for x, y in zip(mixed[2:], flat[2:]))


# ---- 2. the cube map with explicit directions ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cube_case(R):
    g = torch.Generator().manual_seed(5 + R)
    dirs = PO.cubemap_directions(R)
    base = torch.rand(6, R, R, 3, generator=g) * 2 - 0.5
    v_out = torch.randn(dirs.shape[0], 3, generator=g)
    return dirs, base, v_out


def _cube_formulation(R, dtype):
    dirs, base, v_out = _cube_case(R)
    b = base.clone().to(dtype).requires_grad_(True)
    out = PO.cubemap(b, dirs.to(dtype))
    (grad,) = torch.autograd.grad(out, b, v_out.to(dtype))
    return out.detach(), grad


@pytest.mark.parametrize("R", [1, 2, 4, 16])
def test_cubemap_forward_and_backward(R):
    dirs, base, v_out = _cube_case(R)
    M = dirs.shape[0]
    d, b, v = dirs.to(DEV), base.to(DEV), v_out.to(DEV)
    bufs = {"out": _carved((M, 3)), "g_base": _carved((6, R, R, 3), fill=0x00)}
    L.call("gspl_cubemap_fwd", M, R, L.ptr(d), L.ptr(b), L.ptr(bufs["out"][1]), L.stream())
    L.call("gspl_cubemap_bwd", M, R, L.ptr(d), L.ptr(v), L.ptr(bufs["g_base"][1]), L.stream())
    _guards_intact(bufs)
    out, g_base = bufs["out"][1], bufs["g_base"][1]

    (ref_out, ref_grad), (f32_out, f32_grad) = _cube_formulation(R, torch.float64), _cube_formulation(R, torch.float32)
    texel, weight = PO.cube_taps(dirs.double(), R)
    out_sums = (weight[..., None] * base.double().abs().reshape(-1, 3)[texel]).sum(1)
    _judge(f"cubemap R={R} forward", out, f32_out, ref_out, out_sums)
    _judge(f"cubemap R={R} texture gradient", g_base, f32_grad, ref_grad, PO.cubemap_grad_sums(R, dirs, v_out).reshape(6, R, R, 3))
    degenerate = ~torch.isfinite(dirs).all(1) | (dirs == 0).all(1)
    assert int(degenerate.sum()) == 2 and not bool(out.cpu()[degenerate].any())

    # the op gives the same numbers; the gradient is the same sum in another order
    leaf = b.clone().requires_grad_(True)
    got = ops.cubemap_sample(leaf, d)
    assert torch.equal(got.detach(), out)
    got.backward(v)
    assert _ratio(leaf.grad, g_base, PO.cubemap_grad_sums(R, dirs, v_out).reshape(6, R, R, 3)) <= _reorder_bound(texel, weight)

    # every sample's weights sum to 1, and a constant texture comes back everywhere: a lost or doubled seam tap shows here
    live = ~degenerate
    ones = ops.cubemap_sample(torch.ones(6, R, R, 3, device=DEV), d).cpu()
    # (rounding: four products and, at a corner, the renormalisation's reciprocal and products: 8 x 2^-24 on the sum of the
    # weights; the four fused multiply-adds of the sample add half an ulp each)
    assert float((ones[live] - 1).abs().max()) <= 8 * PO.F32_EPS
    const = ops.cubemap_sample(torch.full((6, R, R, 3), 0.37, device=DEV), d).cpu()
    assert float((const[live] - 0.37).abs().max()) <= 12 * PO.F32_EPS * 0.37
    total = torch.ones(6, R, R, 3, device=DEV, requires_grad=True)
    ops.cubemap_sample(total, d).sum().backward()
    assert abs(float(total.grad.double().sum()) - 3 * int(live.sum())) <= 1e-5 * 3 * int(live.sum())
    shaped = ops.cubemap_sample(b[None], d[:1600].reshape(2, 20, 40, 3))
    assert shaped.shape == (2, 20, 40, 3) and torch.equal(shaped.reshape(-1, 3), out[:1600])


def test_envlight_module_and_the_nvdiffrast_stand_in():
    """The call `EnvLight.forward` makes — `texture(base[None], l [1, 1, M, 3] or [B, H, W, 3], filter_mode='linear',
    boundary_mode='cube')` after the axis swap — through the stand-in of gspl_amd.compat, and `HipEnvLight`: the op's numbers and
    gradient, in the caller's shape."""
    from gspl_amd import compat
    from gspl_amd.envlight import HipEnvLight
    R = 4
    dirs, base, v_out = _cube_case(R)
    world = dirs[:1600].to(DEV)
    sky = HipEnvLight(resolution=R).to(DEV)
    with torch.no_grad():
        sky.base.copy_(base.to(DEV))
    swapped = torch.stack([world[:, 0], world[:, 2], -world[:, 1]], dim=-1)
    want = ops.cubemap_sample(sky.base.detach(), swapped)
    # the reference's forward, line by line, on the stand-in
    to_opengl = torch.tensor([[1, 0, 0], [0, 0, 1], [0, -1, 0]], dtype=torch.float32, device=DEV)
    for l in (world, world.reshape(2, 20, 40, 3)):
        m = (l.reshape(-1, 3) @ to_opengl.T).reshape(*l.shape).contiguous()
        prefix = m.shape[:-1]
        if len(prefix) != 3:
            m = m.reshape(1, 1, -1, m.shape[-1])
        light = compat._texture(sky.base[None, ...], m, filter_mode="linear", boundary_mode="cube").view(*prefix, -1)
        assert light.shape == l.shape and torch.equal(light.detach().reshape(-1, 3), want)
        assert torch.equal(sky(l).detach(), light.detach())
    light.backward(v_out[:1600].to(DEV).reshape(2, 20, 40, 3))
    ref = sky.base.detach().clone().requires_grad_(True)
    ops.cubemap_sample(ref, swapped).backward(v_out[:1600].to(DEV))
    texel, weight = PO.cube_taps(swapped.cpu().double(), R)
    sums = PO.cubemap_grad_sums(R, swapped.cpu(), v_out[:1600]).reshape(6, R, R, 3)
    assert float(sky.base.grad.abs().max()) > 0 and _ratio(sky.base.grad, ref.grad, sums) <= _reorder_bound(texel, weight)


# ---- 3. the fused blend -----------------------------------------------------------------------------------------------------------------
FX, FY = 12.0, 11.5          # 37x50 pixels then span about +-64 degrees: three faces


@functools.lru_cache(maxsize=None)
def _blend_case(H, W, R, jittered):
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + R + (1 if jittered else 0))
    rgb, alpha = torch.rand(3, H, W, generator=g), torch.rand(H, W, generator=g)
    alpha[0, 0] = 1.0
    base = torch.rand(6, R, R, 3, generator=g) * 2 - 0.5
    jitter = torch.rand(2, H, W, generator=g) if jittered else None
    v_out = torch.randn(3, H, W, generator=g)
    return rgb, alpha, base, jitter, v_out, W / 2 + 0.3, H / 2 - 0.2


@pytest.mark.parametrize("jittered", [False, True], ids=["centres", "jitter"])
@pytest.mark.parametrize("rot", range(6))
@pytest.mark.parametrize("R", [2, 16])
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (37, 50)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_blend_forward_and_backward(hw, R, rot, jittered):
    H, W = hw
    rgb, alpha, base, jitter, v_out, cx, cy = _blend_case(H, W, R, jittered)
    rot64 = PO.rotations()[rot]
    rot32 = rot64.float()
    to = lambda x: None if x is None else x.to(DEV)
    table = ops.envlight.blend_table(to(rot32), torch.tensor(FX, device=DEV), FY, torch.tensor(cx, device=DEV), cy, DEV)
    assert table.shape == (13,)
    d_rgb, d_alpha, d_base, d_jit, d_v = to(rgb), to(alpha), to(base), to(jitter), to(v_out)
    bufs = {"out": _carved((3, H, W)), "dirs": _carved((H, W, 3)), "g_alpha": _carved((H, W)), "g_base": _carved((6, R, R, 3), fill=0x00)}
    out, dirs, g_alpha, g_base = (bufs[k][1] for k in ("out", "dirs", "g_alpha", "g_base"))
    L.call("gspl_envlight_blend_fwd", H, W, R, L.ptr(table), L.ptr(d_rgb), L.ptr(d_alpha), L.ptr(d_base), L.ptr(d_jit), L.ptr(out),
           L.ptr(dirs), L.stream())
    L.call("gspl_envlight_blend_bwd", H, W, R, L.ptr(table), L.ptr(d_alpha), L.ptr(d_base), L.ptr(d_jit), L.ptr(d_v), L.ptr(g_alpha),
           L.ptr(g_base), L.stream())
    _guards_intact(bufs)
    dirs_cpu = dirs.cpu()

    # the directions against the fp64 formula (the inputs are the float32 table's values)
    scal = [float(torch.tensor(x, dtype=torch.float32)) for x in (FX, FY, cx, cy)]
    ref_dirs = PO.pixel_directions(rot32.double(), *scal, H, W, None if jitter is None else jitter.double())
    f32_dirs = PO.pixel_directions(rot32, *[torch.tensor(x, dtype=torch.float32) for x in scal], H, W, jitter)
    cam = PO.pixel_directions(torch.eye(3, dtype=torch.float64), *scal, H, W, None if jitter is None else jitter.double())
    cam = torch.stack([cam[..., 0], -cam[..., 2], cam[..., 1]], -1)          # (the swap undone: the camera-space unit vector)
    swap = lambda m: torch.stack([m[0], m[2], m[1]])
    dir_sums = cam.abs() @ swap(rot32.double().abs()).T
    _judge(f"blend {H}x{W} rot={rot} directions", dirs_cpu, f32_dirs, ref_dirs, dir_sums)

    # the oracle is fed the kernel's own directions, widened exactly: the face choice cannot differ
    def formulation(dtype):
        r, a, b = (x.clone().to(dtype).requires_grad_(True) for x in (rgb, alpha, base))          # (the case's tensors are shared: copies)
        res = PO.blend(r, a, b, dirs_cpu.to(dtype))
        return (res.detach(),) + torch.autograd.grad(res, (r, a, b), v_out.to(dtype))

    ref, f32 = formulation(torch.float64), formulation(torch.float32)
    flat_dirs = dirs_cpu.double().reshape(-1, 3)
    texel, weight = PO.cube_taps(flat_dirs, R)
    sky_abs = (weight[..., None] * base.double().abs().reshape(-1, 3)[texel]).sum(1).reshape(H, W, 3).permute(2, 0, 1)
    T = (1 - alpha.double())
    tag = f"blend {H}x{W} R={R} rot={rot} {'jitter' if jittered else 'centres'}"
    _judge(f"{tag} forward", out, f32[0], ref[0], rgb.double().abs() + T[None] * sky_abs)
    assert torch.equal(ref[1], v_out.double())
    _judge(f"{tag} g_alpha", g_alpha, f32[2], ref[2], (v_out.double().abs() * sky_abs).sum(0))
    upstream_at_texels = (T[None] * v_out.double()).permute(1, 2, 0).reshape(-1, 3)
    _judge(f"{tag} texture gradient", g_base, f32[3], ref[3], PO.cubemap_grad_sums(R, flat_dirs, upstream_at_texels).reshape(6, R, R, 3))

    # the op: the same numbers; g_rgb is the upstream gradient bit for bit
    leaves = [x.clone().requires_grad_(True) for x in (d_rgb, d_alpha, d_base)]
    got, got_dirs = ops.envlight_blend(*leaves, to(rot32), torch.tensor(FX, device=DEV), FY, torch.tensor(cx, device=DEV), cy, d_jit,
                                       return_dirs=True)
    assert torch.equal(got.detach(), out) and torch.equal(got_dirs, dirs) and not got_dirs.requires_grad
    got.backward(d_v)
    assert torch.equal(leaves[0].grad, d_v) and torch.equal(leaves[1].grad, g_alpha)
    assert _ratio(leaves[2].grad, g_base, PO.cubemap_grad_sums(R, flat_dirs, upstream_at_texels).reshape(6, R, R, 3)) <= _reorder_bound(texel, weight)

    # fused against unfused
    sky = ops.cubemap_sample(d_base, dirs).permute(2, 0, 1)
    unfused = d_rgb + (1 - d_alpha)[None] * sky
    assert bool(((out - unfused).abs() <= 2 * PO.F32_EPS * (d_rgb.abs() + sky.abs())).all())
    assert torch.equal(out[:, 0, 0], d_rgb[:, 0, 0])          # alpha == 1: the sky does not show


def test_three_faces_are_in_view():
    """The 37x50 frame of the blend cases looks at three faces at least (for every rotation)."""
    for rot in PO.rotations():
        dirs = PO.pixel_directions(rot, FX, FY, 25.3, 18.3, 37, 50)
        assert len(torch.unique(PO.select_face(dirs.reshape(-1, 3))[0])) >= 3


# ---- 4. the renderer --------------------------------------------------------------------------------------------------------------------
W_, H_ = 64, 48


def _renderer_scene(env_map_res):
    from gspl_amd.renderers import HipPeriodicVibrationGaussianRenderer
    scene = PO.pvg_scene(200)
    model = PO.FakePVGModel(**{k: v.to(DEV) for k, v in scene.items()})
    cam = O.synthetic_camera(W_, H_, 60.0, 58.0)
    camera = FakeCamera(cam, DEV)
    camera.time = torch.tensor(TIME, device=DEV)
    renderer = HipPeriodicVibrationGaussianRenderer(env_map_res=env_map_res).instantiate()
    renderer.setup("fit")
    renderer.to(DEV).eval()
    if env_map_res > 0:
        with torch.no_grad():
            g = torch.Generator().manual_seed(3)
            renderer.env_map.base.copy_(torch.rand(6, env_map_res, env_map_res, 3, generator=g))
    return scene, model, cam, camera, renderer


def _stages(model, camera, shift=None):
    """The renderer's own stages, op by op: what it hands to the compositing pass."""
    from gspl_amd.renderers.hip_gsplat_renderer import _project
    scale_t = model.get_scale_t()
    means_t, avg_v, op_t = ops.pvg_motion(model.get_means(), model.get_velocity(), model.get_t(), scale_t, model.get_opacities(), camera.time,
                                          CYCLE, DECAY, OFFSET, shift)
    xys, depths, radii, conics, comp, tiles, _ = _project(means_t, model.get_scaling, model.get_rotation, camera, 1.0, 16, W_, H_)
    opac = op_t * comp[:, None]
    rgbs = ops.sh_view_colors(model.active_sh_degree, model.get_xyz, camera.camera_center, model.get_features, None, radii > 0)
    isects = ops.bin_gaussians(xys, depths, radii, H_, W_, 16, conics=conics, opacities=opac)
    return dict(xys=xys, depths=depths, radii=radii, conics=conics, tiles=tiles, opac=opac, rgbs=rgbs, avg_v=avg_v, scale_t=scale_t,
                isects=isects)


@pytest.mark.parametrize("env_map_res", [0, 4])
def test_renderer_maps_are_slices_of_one_pass(env_map_res):
    scene, model, cam, camera, renderer = _renderer_scene(env_map_res)
    bg = torch.tensor([0.1, 0.3, 0.6], device=DEV)
    types = ["rgb", "rgb_without_envmap", "depth", "alpha", "average_velocity", "scale_t"]
    with torch.no_grad():
        out = renderer(camera, model, bg, render_types=types)
        s = _stages(model, camera)
        sep = lambda colors, background, **kw: ops.rasterize_gaussians(
            s["xys"], s["depths"], s["radii"], s["conics"], s["tiles"], colors, s["opac"], H_, W_, 16, background=background,
            isects=s["isects"], channels_first=True, **kw)
        zero3, zero1 = torch.zeros(3, device=DEV), torch.zeros(1, device=DEV)
        rgb, alpha = sep(s["rgbs"], bg, return_alpha=True)
        # BIT equality, channel group by channel group
        assert torch.equal(out["rgb_without_envmap"], rgb) and torch.equal(out["alpha"], alpha[None])
        assert torch.equal(out["average_velocity"], sep(s["avg_v"], zero3))
        assert torch.equal(out["depth"], sep(s["depths"][:, None], zero1))
        assert torch.equal(out["scale_t"], sep(s["scale_t"], zero1))
        assert float(alpha.max()) > 0.3 and float(alpha.min()) < 0.05 and torch.equal(out["radii"], s["radii"])
        if env_map_res > 0:
            from gspl_amd.renderers.hip_pvg_renderer import camera_to_world_rotation
            want = ops.envlight_blend(rgb, alpha, renderer.env_map.base, camera_to_world_rotation(camera), camera.fx, camera.fy, camera.cx,
                                      camera.cy)
            assert torch.equal(out["render"], want) and not torch.equal(out["render"], rgb)
        else:
            assert renderer.env_map is None and torch.equal(out["render"], rgb)
        # fewer maps: the narrow passes, the same numbers
        few = renderer(camera, model, bg, render_types=["rgb", "depth"])
        assert torch.equal(few["render"], out["render"]) and torch.equal(few["depth"], out["depth"])
        assert few["average_velocity"] is None and few["scale_t"] is None
        only_depth = renderer(camera, model, bg, render_types=["depth"])
        assert only_depth["render"] is None and torch.equal(only_depth["depth"], out["depth"])
        unknown = renderer(camera, model, bg, render_types=["normal"])
        assert all(unknown[k] is None for k in ("render", "rgb_without_envmap", "depth", "alpha", "average_velocity", "scale_t"))
        assert list(unknown) == list(out) and torch.equal(unknown["radii"], out["radii"])
        only_velocity = renderer(camera, model, bg, render_types=["average_velocity"])
        assert only_velocity["render"] is None and torch.equal(only_velocity["average_velocity"], out["average_velocity"])
    assert out["viewspace_points"].shape == (200, 2) and out["visibility_filter"].dtype == torch.bool
    assert torch.equal(out["viewspace_points_grad_scale"].cpu(), 0.5 * torch.tensor([[W_, H_]], dtype=torch.float32))


@pytest.mark.parametrize("shifted", [False, True], ids=["unshifted", "shifted"])
@pytest.mark.parametrize("env_map_res", [0, 4])
def test_renderer_gradients_against_fp64(env_map_res, shifted):
    from gspl_amd.renderers.hip_pvg_renderer import camera_to_world_rotation
    scene, model, cam, camera, renderer = _renderer_scene(env_map_res)
    shift = SHIFT if shifted else None
    bg = torch.tensor([0.1, 0.3, 0.6])
    g = torch.Generator().manual_seed(9)
    gt = torch.rand(3, H_, W_, generator=g)

    # the fp64 pipeline, its compositing evaluated on the implementation's lists and per-splat values
    with torch.no_grad():
        s = _stages(model, camera, shift)
    dl = {k: v.double().requires_grad_(True) for k, v in scene.items()}
    time = float(torch.tensor(TIME, dtype=torch.float32))
    means_t, avg_v, op_t = PO.motion(dl["means"], dl["velocity"], dl["t"], dl["scale_t"], dl["opacities"], time, OFFSET, shift, CYCLE, DECAY)
    xys, depths, radii, conics, comp = O.project_gaussians(means_t, dl["scales"], 1.0, dl["quats"], cam["world_to_camera"].double(), cam["fx"],
                                                          cam["fy"], cam["cx"], cam["cy"], H_, W_)[:5]
    assert np.array_equal(radii.numpy(), s["radii"].cpu().numpy())
    rgbs = O.sh_colors(3, dl["shs"], dl["means"], cam["camera_center"].double(), detach_dirs=True)
    colors = torch.cat([rgbs, avg_v, depths[:, None], dl["scale_t"]], dim=1)
    impl_colors = torch.cat([s["rgbs"], s["avg_v"], s["depths"][:, None], s["scale_t"]], dim=1)
    flat, offs = s["isects"]
    bg8 = torch.cat([bg, torch.zeros(5)]).double()
    image, alpha, fragile = O.composite_locked(O.MODE_GSPLAT, (xys, conics, colors, op_t[:, 0] * comp),
                                               [x.cpu() for x in (s["xys"], s["conics"], impl_colors, s["opac"])], bg8, W_, H_,
                                               offs.cpu().numpy(), flat.cpu().numpy())
    firm = ~fragile
    assert float(firm.double().mean()) > 0.99
    image = image.permute(2, 0, 1)
    render = image[0:3]
    base64 = None
    if env_map_res > 0:
        base64 = renderer.env_map.base.detach().cpu().double().requires_grad_(True)
        with torch.no_grad():
            _, dirs = ops.envlight_blend(torch.zeros(3, H_, W_, device=DEV), torch.zeros(H_, W_, device=DEV), renderer.env_map.base,
                                         camera_to_world_rotation(camera), camera.fx, camera.fy, camera.cx, camera.cy, return_dirs=True)
        render = PO.blend(render, alpha, base64, dirs.cpu().double())

    def loss_of(render, velocity_map, alpha, gt, firm):
        l1 = ((render - gt).abs() * firm).mean()
        v_reg = ((velocity_map / alpha.detach().clamp_min(1e-5)).abs() * firm).mean() * 0.001
        return 0.8 * l1 + v_reg

    loss_of(render, image[3:6], alpha[None], gt.double(), firm[None]).backward()

    out = renderer(camera, model, bg.to(DEV), time_shift=shift)          # the default render types: rgb and average_velocity
    assert out["depth"] is None and out["scale_t"] is None
    loss = loss_of(out["render"], out["average_velocity"], out["alpha"], gt.to(DEV), firm[None].to(DEV))
    loss.backward()
    print(f"loss {float(loss):.6f} (fp64 {float(loss_of(render, image[3:6], alpha[None], gt.double(), firm[None])):.6f}), "
          f"{int(fragile.sum())} fragile pixels")
    for name, leaf in model.leaves().items():
        ref = dl[name].grad
        assert float(ref.abs().max()) > 0, name
        assert_close_scaled(leaf.grad.cpu().numpy(), ref.numpy(), 1e-4, f"{name}.grad", frac_ok=1.0)
    if env_map_res > 0:
        assert float(base64.grad.abs().max()) > 0
        assert_close_scaled(renderer.env_map.base.grad.cpu().numpy(), base64.grad.numpy(), 1e-4, "base.grad", frac_ok=1.0)


def test_renderer_with_the_configuration_of_pvg_dynamic_yaml():
    """env_map_res = -1 and lambda_self_supervision = -1: no sky, never a time shift; the output keys are the reference's."""
    from gspl_amd.renderers import HipPeriodicVibrationGaussianRenderer
    names = json.load(open(os.path.join(ROOT, "tests", "golden", "pvg_renderer_signatures.json")))
    scene, model, cam, camera, _ = _renderer_scene(0)
    renderer = HipPeriodicVibrationGaussianRenderer(env_map_res=-1, lambda_self_supervision=-1).instantiate()
    renderer.setup("fit")
    renderer.to(DEV)
    assert renderer.env_map is None and renderer.training
    renderer.time_interval = 0.02
    assert abs(renderer.time_interval - 0.02) < 1e-8 and "_time_interval" in renderer.state_dict()
    bg = torch.zeros(3, device=DEV)
    out = renderer.training_forward(0, None, camera, model, bg)
    assert list(out) == names["output_keys"]
    assert out["render"].shape == (3, H_, W_) and out["average_velocity"].shape == (3, H_, W_) and out["alpha"].shape == (1, H_, W_)
    with torch.no_grad():
        unshifted = renderer(camera, model, bg)
    assert torch.equal(out["render"].detach(), unshifted["render"])          # lambda_self_supervision = -1: never shifted
    shifted = renderer(camera, model, bg, time_shift=0.03)
    assert not torch.equal(shifted["render"].detach(), unshifted["render"])


def test_training_mode_jitters_the_sky_only():
    scene, model, cam, camera, renderer = _renderer_scene(4)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        still = renderer(camera, model, bg)
        renderer.train()
        a, b = renderer(camera, model, bg), renderer(camera, model, bg)
    assert torch.equal(a["rgb_without_envmap"], still["rgb_without_envmap"]) and torch.equal(a["alpha"], still["alpha"])
    assert not torch.equal(a["render"], b["render"]) and float((a["render"] - still["render"]).abs().max()) < 1.0


def test_camera_time_on_the_device_needs_no_host_synchronisation():
    scene, model, cam, camera, renderer = _renderer_scene(4)
    from gspl_amd.renderers.hip_pvg_renderer import camera_to_world_rotation
    rot = camera_to_world_rotation(camera)
    rgb, alpha = torch.rand(3, H_, W_, device=DEV), torch.rand(H_, W_, device=DEV, requires_grad=True)
    jitter = torch.rand(2, H_, W_, device=DEV)

    def step(shift):
        outs = ops.pvg_motion(model.get_means(), model.get_velocity(), model.get_t(), model.get_scale_t(), model.get_opacities(), camera.time,
                              CYCLE, DECAY, OFFSET, shift)
        sky = ops.envlight_blend(rgb, alpha, renderer.env_map.base, rot, camera.fx, camera.fy, camera.cx, camera.cy, jitter)
        (sum(o.sum() for o in outs) + sky.sum()).backward()

    step(SHIFT)          # (loads the kernels; the model's constants are written to the device once per model)
    for p in list(model.parameters()) + [renderer.env_map.base, alpha]:
        p.grad = None
    assert camera.time.is_cuda
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        # training draws a new time_shift on every shifted step: values never seen before, a python time, and no shift at all
        for shift in (0.00731, -0.0213, None, 0.0004):
            step(shift)
        ops.pvg_motion(model.get_means(), model.get_velocity(), model.get_t(), model.get_scale_t(), model.get_opacities(), 0.4321, CYCLE, DECAY,
                       OFFSET, 0.0111)
        ops.envlight_blend(rgb, alpha, renderer.env_map.base, rot, 61.5, 59.25, 31.0, 23.5)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    from gspl_amd.ops import pvg as pvg_module
    assert all(len(key) == 3 for key in pvg_module._CONSTANTS), "the kept constants must not be keyed on the shift"
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.leaves().values())
    assert float(renderer.env_map.base.grad.abs().max()) > 0 and float(alpha.grad.abs().max()) > 0

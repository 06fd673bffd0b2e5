"""The SH colour kernels (csrc/sh.hip) on the paths the other SH tests leave out: the means gradient of the fused colour launch
(origin, +0.5 / clamp, mask and the normalisation d = v / |v| together), an upstream gradient that is a column block of a wider
buffer, coefficient tensors whose base is not 16-byte aligned (the scalar staging path), block edges and the over-64-KiB LDS
branch, and through the C ABI unaligned gradient outputs and padded row strides.

The reference throughout is oracle.gsplat_oracle in fp64, autograd included.  Where two GPU runs perform the same arithmetic and
differ only in how rows are loaded or stored (aligned / unaligned, dense / strided, dense / padded) they are compared bit for bit.

Clamp: a channel whose SH + 0.5 lies within 1e-5 of zero ("fragile") may legitimately clamp on one side and not on the other, which
switches its whole gradient; rows with such a channel are left out of the gradient comparison (only those), and every test that
uses the clamp first asserts on the fp64 reference alone that they are rare and that both sides of the clamp are well populated."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gspl_amd  # noqa: F401
from gspl_amd import _lib as L
from gspl_amd import ops

from oracle import gsplat_oracle as O
from hip_helpers import assert_close_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

N_RAGGED = 1031                       # ragged against the 256-row block
CASES = [(0, 1), (0, 16), (1, 4), (1, 16), (2, 9), (2, 16), (3, 16), (4, 25)]       # (degree, coefficients per splat)
CENTER = (0.3, -0.2, 4.0)
SENTINEL = 12345.0
BAND = 1024                           # sentinel floats on each side of a C-ABI buffer
# one seed per N: found on the fp64 reference alone (the clamp / fragile shares asserted by `_clamp_shares`; with N = 1 there are three
# live channels, of which one or two must clamp)
SEEDS = {1: 3, 255: 7, 256: 7, 257: 7, 513: 7, 1031: 7}


def _inputs(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    means = torch.randn(N, 3, generator=g) * 1.5
    center = torch.tensor(CENTER)
    # every fifth splat close to the camera: |means - center| in [0.05, 0.5] — the 1 / |v| factor of the means gradient
    u = torch.randn(N, 3, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    r = 0.05 + 0.45 * torch.rand(N, generator=g)
    near = torch.arange(N) % 5 == 0
    means = torch.where(near[:, None], center + u * r[:, None], means)
    dc = torch.randn(N, 1, 3, generator=g) * 2.0
    rest = torch.randn(N, K - 1, 3, generator=g) * 0.5
    w = torch.randn(N, 3, generator=g)
    mask = torch.rand(N, generator=g) > 0.3
    return means, center, dc, rest, w, mask


def _clamp_shares(raw, live, what):
    """raw: SH + 0.5 before the clamp in fp64 [..., 3]; live [...] bool.  Asserted on the reference alone: at least 2 % of the live
    channels clamp, at least 2 % do not, at most 0.1 % are fragile.  Returns the fragile channels [..., 3]."""
    raw, live = raw.detach(), live.bool()
    assert bool(live.any()), f"{what}: no live row"
    ch = raw[live]
    clamp, fragile = float((ch < 0).double().mean()), float((ch.abs() < 1e-5).double().mean())
    print(f"[clamp] {what}: {ch.numel()} live channels, {100 * clamp:.2f} % clamp, {100 * fragile:.3f} % fragile")
    assert clamp >= 0.02 and 1.0 - clamp >= 0.02, f"{what}: {clamp:.4f} of the live channels clamp"
    assert fragile <= 1e-3, f"{what}: {fragile:.5f} of the live channels are fragile"
    return (raw.abs() < 1e-5) & live[..., None]


@functools.lru_cache(maxsize=None)
def _view_reference(N, K, seed, degree, masked):
    """fp64 reference of sh_view_colors(detach_means=False) under the loss (colours * w).sum(): colours (zero where masked), the
    gradients of means and coefficients, the rows with a fragile channel.  Computed once per case and shared; callers do not
    modify what it returns."""
    means, center, dc, rest, w, mask = _inputs(N, K, seed)
    live = mask if masked else torch.ones(N, dtype=torch.bool)
    m = means.double().requires_grad_(True)
    co = torch.cat([dc, rest], 1).double().requires_grad_(True)
    raw = O.eval_sh(degree, co.detach(), means.double() - center.double()) + 0.5
    fragile = _clamp_shares(raw, live, f"N={N} K={K} degree={degree} masked={masked}").any(-1).numpy()
    col = torch.where(live[:, None], O.sh_colors(degree, co, m, center.double(), detach_dirs=False), torch.zeros((), dtype=torch.float64))
    (col * w.double()).sum().backward()
    v_means = torch.zeros_like(means, dtype=torch.float64) if m.grad is None else m.grad          # (degree 0: no path to the means)
    return dict(col=col.detach().numpy(), v_means=v_means.numpy(), v_coeffs=co.grad.numpy(), fragile=fragile, live=live.numpy())


def _leaf(t):
    return t.clone().to(DEV).requires_grad_(True)


def _coeff_leaves(dc, rest, merged):
    """(dc, rest) as the ops take them: the merged [N,K,3] tensor with rest None, or the model's two tensors."""
    if merged:
        return _leaf(torch.cat([dc, rest], 1)), None
    return _leaf(dc), _leaf(rest)


def _coeff_grad(dc, rest):
    return (dc.grad if rest is None else torch.cat([dc.grad, rest.grad], 1)).cpu()


def _view_run(degree, means, center, dc, rest, mask, w, merged):
    """One forward and backward of sh_view_colors(detach_means=False) -> colours, means gradient, coefficient gradient [N,K,3] (CPU)."""
    m = _leaf(means)
    d, r = _coeff_leaves(dc, rest, merged)
    col = ops.sh_view_colors(degree, m, center.to(DEV), d, r, None if mask is None else mask.to(DEV), detach_means=False)
    (col * w.to(DEV)).sum().backward()
    return col.detach().cpu(), m.grad.cpu(), _coeff_grad(d, r)


def _check_view_against_fp64(got, ref, degree, K, what):
    col, v_means, v_coeffs = got
    np.testing.assert_allclose(col.numpy(), ref["col"], rtol=2e-5, atol=3e-6, err_msg=f"{what}: colours")
    keep = ~ref["fragile"]
    np.testing.assert_allclose(v_coeffs.numpy()[keep], ref["v_coeffs"][keep], rtol=2e-5, atol=3e-6, err_msg=f"{what}: coefficient gradient")
    assert_close_scaled(v_means.numpy()[keep], ref["v_means"][keep], 2e-4, "v_means")
    assert torch.all(v_means[~torch.from_numpy(ref["live"])] == 0), f"{what}: a masked row has a means gradient"
    assert torch.all(v_coeffs[~torch.from_numpy(ref["live"])] == 0), f"{what}: a masked row has a coefficient gradient"
    assert torch.all(v_coeffs[:, (degree + 1) ** 2:] == 0), f"{what}: a gradient above the active degree"
    if degree == 0:
        assert torch.all(v_means == 0), f"{what}: degree 0 does not depend on the direction"


# ---------------------------------------------------------------------------------------------
# 1. the means gradient of the fused colour launch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("merged", [True, False], ids=["merged", "decomposed"])
@pytest.mark.parametrize("degree,K", CASES)
def test_view_colors_means_gradient_vs_fp64(degree, K, merged, masked):
    """sh_bwd_kernel<DEG, WITH_DIRS> without a Jacobian, as HipSWAGRenderer and HipVanillaRenderer(convert_SHs_python=True) run it:
    origin subtracted, gradient masked by `clamped` and by the mask, and taken through d = v / |v|."""
    N, seed = N_RAGGED, SEEDS[N_RAGGED]
    means, center, dc, rest, w, mask = _inputs(N, K, seed)
    ref = _view_reference(N, K, seed, degree, masked)
    got = _view_run(degree, means, center, dc, rest, mask if masked else None, w, merged)
    _check_view_against_fp64(got, ref, degree, K, f"degree {degree} K {K}")
    if degree == 0 and K > 1:
        # the colour is the DC term alone: the same launch on the DC rows only
        alone = ops.sh_view_colors(0, means.to(DEV), center.to(DEV), dc.to(DEV), None, mask.to(DEV) if masked else None)
        assert torch.equal(got[0], alone.cpu())


# ---------------------------------------------------------------------------------------------
# the gsplat signature: un-normalised directions, no origin, no clamp — with masks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merged", [True, False], ids=["merged", "decomposed"])
@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_gsplat_signature_dirs_gradient_with_masks(degree, merged):
    N, K = N_RAGGED, (degree + 1) ** 2
    means, center, dc, rest, w, mask = _inputs(N, K, SEEDS[N])
    dirs0 = 2.5 * (means - center)
    dirs = _leaf(dirs0)
    d, r = _coeff_leaves(dc, rest, merged)
    if merged:
        col = ops.spherical_harmonics(degree, dirs, d, mask.to(DEV))
    else:
        col = ops.spherical_harmonics_decomposed(degree, dirs, d, r, mask.to(DEV))
    (col * w.to(DEV)).sum().backward()

    dd = dirs0.double().requires_grad_(True)
    co = torch.cat([dc, rest], 1).double().requires_grad_(True)
    ref = torch.where(mask[:, None], O.eval_sh(degree, co, dd), torch.zeros((), dtype=torch.float64))
    (ref * w.double()).sum().backward()
    np.testing.assert_allclose(col.detach().cpu().numpy(), ref.detach().numpy(), rtol=2e-5, atol=3e-6)
    np.testing.assert_allclose(_coeff_grad(d, r).numpy(), co.grad.numpy(), rtol=2e-5, atol=3e-6)
    assert_close_scaled(dirs.grad.cpu().numpy(), dd.grad.numpy(), 2e-4, "v_dirs")
    assert torch.all(dirs.grad.cpu()[~mask] == 0) and torch.all(col.detach().cpu()[~mask] == 0)
    assert torch.all(_coeff_grad(d, r)[~mask] == 0)


# ---------------------------------------------------------------------------------------------
# 2. a strided upstream gradient
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merged", [True, False], ids=["merged", "decomposed"])
def test_strided_upstream_gradient_is_consumed_in_place(merged):
    """The colours go into a concat (HipSWAGRenderer: [colours, x_emb, image_emb], 19 columns), whose backward hands the SH backward
    a `narrow` view: row stride 4 or 19, read in place through `v_colors_stride`.  Same numbers, same arithmetic as the dense
    gradient — only the loads differ — so the results are equal bit for bit.  A transposed gradient is one `_rows` must copy."""
    degree, K, N = 3, 16, N_RAGGED
    means, center, dc, rest, w, mask = _inputs(N, K, SEEDS[N])
    _view_reference(N, K, SEEDS[N], degree, True)            # (the clamp / fragile shares of these inputs)
    g = torch.Generator().manual_seed(5)

    def run(upstream):
        m = _leaf(means)
        d, r = _coeff_leaves(dc, rest, merged)
        col = ops.sh_view_colors(degree, m, center.to(DEV), d, r, mask.to(DEV), detach_means=False)
        seen = []
        col.register_hook(lambda v: seen.append((tuple(v.shape), tuple(v.stride()))))
        upstream(col)
        return (m.grad.cpu(), _coeff_grad(d, r)), seen[0]

    dense, layout = run(lambda col: col.backward(w.to(DEV)))
    assert layout == ((N, 3), (3, 1))
    for extra in (1, 16):
        W = torch.cat([w, torch.randn(N, extra, generator=g)], 1).to(DEV)
        other = torch.randn(N, extra, generator=g).to(DEV)
        got, layout = run(lambda col: (torch.cat([col, other], -1) * W).sum().backward())
        assert layout == ((N, 3), (3 + extra, 1)), "the SH backward was not handed a column block of the wider gradient"
        for a, b, name in zip(got, dense, ("means", "coefficients")):
            assert torch.equal(a, b), f"row stride {3 + extra}: the {name} gradient differs from the dense run's"
    wt = w.t().contiguous().to(DEV)
    got, layout = run(lambda col: (col.t() * wt).sum().backward())
    assert layout == ((N, 3), (1, N)), "the SH backward was not handed a transposed gradient"
    for a, b, name in zip(got, dense, ("means", "coefficients")):
        assert torch.equal(a, b), f"transposed upstream gradient: the {name} gradient differs from the dense run's"


# ---------------------------------------------------------------------------------------------
# 3. the scalar staging path
# ---------------------------------------------------------------------------------------------
def _carve(t, offset):
    """`t` as a contiguous view that starts `offset` floats into a fresh flat buffer (a leaf that requires a gradient)."""
    flat = torch.zeros(t.numel() + 8, dtype=torch.float32, device=DEV)
    view = flat[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    if t.numel():
        assert view.data_ptr() % 16 == 4 * offset and view.is_contiguous()
    return view.requires_grad_(True)


_CENTERS = torch.tensor([CENTER, (1.3, -0.2, 4.0), (0.3, -1.2, 4.5)])


def _all_ops(degree, means, center, dc, rest, w, mask, radii, w3, place):
    """Every SH op that stages coefficient rows, with its coefficient tensors put on the device by `place`: a list of
    (name, [tensors to compare bit for bit])."""
    out = []
    cat = torch.cat([dc, rest], 1)
    # gsplat signature (merged), direction gradient from the coefficients, masked
    dirs, c = _leaf(2.5 * (means - center)), place(cat)
    col = ops.spherical_harmonics(degree, dirs, c, mask.to(DEV))
    (col * w.to(DEV)).sum().backward()
    out.append(("spherical_harmonics", [col.detach(), dirs.grad, c.grad]))
    for merged in (True, False):
        m = _leaf(means)
        d, r = (place(cat), None) if merged else (place(dc), place(rest))
        col = ops.sh_view_colors(degree, m, center.to(DEV), d, r, None, detach_means=False)
        (col * w.to(DEV)).sum().backward()
        out.append((f"sh_view_colors {'merged' if merged else 'decomposed'}", [col.detach(), m.grad, d.grad] + ([] if merged else [r.grad])))
        d, r = (place(cat), None) if merged else (place(dc), place(rest))
        col = ops.sh_view_colors_batched(degree, means.to(DEV), _CENTERS.to(DEV), d, r, radii.to(DEV))
        (col * w3.to(DEV)).sum().backward()
        out.append((f"sh_view_colors_batched {'merged' if merged else 'decomposed'}", [col.detach(), d.grad] + ([] if merged else [r.grad])))
    return out


@pytest.mark.parametrize("N", [1, 255, 256, 257, N_RAGGED])
@pytest.mark.parametrize("degree,K", [(1, 4), (2, 9), (3, 16), (4, 25)])
def test_unaligned_coefficient_bases_take_the_scalar_path(degree, K, N):
    """tile_load takes 16-byte loads only from a 16-byte-aligned base; a contiguous view with a storage offset (coeffs[1:] at K = 9 or
    25, a flat parameter buffer sliced at an odd float) is staged float by float.  Same values in LDS either way, so colours and
    all gradients equal those of aligned clones bit for bit — also the mix of unaligned inputs with aligned (fresh) gradients."""
    seed = SEEDS[N]
    means, center, dc, rest, w, mask = _inputs(N, K, seed)
    g = torch.Generator().manual_seed(100 + N)
    radii = torch.randint(-1, 4, (3, N), generator=g, dtype=torch.int32)
    if N == 1:
        radii[:] = 2
    w3 = torch.randn(3, N, 3, generator=g)
    ref = _view_reference(N, K, seed, degree, False)            # asserts the clamp / fragile shares of the one-camera launches
    cat = torch.cat([dc, rest], 1).double()
    raw3 = torch.stack([O.eval_sh(degree, cat, means.double() - c.double()) + 0.5 for c in _CENTERS])
    _clamp_shares(raw3, radii > 0, f"batched N={N} K={K} degree={degree}")

    aligned = _all_ops(degree, means, center, dc, rest, w, mask, radii, w3, _leaf)
    for offset in (1, 2, 3):
        got = _all_ops(degree, means, center, dc, rest, w, mask, radii, w3, lambda t: _carve(t, offset))
        for (name, a), (_, b) in zip(got, aligned):
            for i, (x, y) in enumerate(zip(a, b)):
                assert torch.equal(x, y), f"{name}, offset {offset} floats: tensor {i} differs from the aligned run's"
    if (degree, K, N) == (3, 16, N_RAGGED):
        # one representative case against fp64 as well: decomposed, base 4 bytes past alignment
        m, d, r = _leaf(means), _carve(dc, 1), _carve(rest, 1)
        col = ops.sh_view_colors(degree, m, center.to(DEV), d, r, None, detach_means=False)
        (col * w.to(DEV)).sum().backward()
        _check_view_against_fp64((col.detach().cpu(), m.grad.cpu(), _coeff_grad(d, r)), ref, degree, K, "unaligned decomposed")


# ---------------------------------------------------------------------------------------------
# 4. block edges
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merged", [True, False], ids=["merged", "decomposed"])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("degree,K", [(0, 1), (0, 16), (3, 16), (4, 25)])
def test_block_edges(degree, K, N, merged):
    """One row, one short of a block, a full block, one over, two blocks and a row.  Degree 4 stages more than 64 KiB of LDS per
    block, which the launcher has to ask for (hipFuncSetAttribute)."""
    if degree == 4:
        floats_per_row = (3 * K) | 1 if merged else (3 * (K - 1)) | 1
        assert 256 * floats_per_row * 4 > 65536 and 256 * ((3 * K) | 1) * 4 > 65536
    seed = SEEDS[N]
    means, center, dc, rest, w, mask = _inputs(N, K, seed)
    ref = _view_reference(N, K, seed, degree, False)
    got = _view_run(degree, means, center, dc, rest, None, w, merged)
    _check_view_against_fp64(got, ref, degree, K, f"N {N} degree {degree} K {K}")


# ---------------------------------------------------------------------------------------------
# the C ABI: unaligned gradient outputs, padded row strides
# ---------------------------------------------------------------------------------------------
def _p(t, offset_floats=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * offset_floats)


class _Banded:
    """`n` floats between two bands of SENTINEL, starting `shift` floats past 16-byte alignment; the inner floats are pre-filled with
    SENTINEL too."""

    def __init__(self, n, shift=0):
        self.n, self.lo = n, BAND + shift
        self.outer = torch.full((BAND + shift + n + BAND,), SENTINEL, dtype=torch.float32, device=DEV)
        assert self.outer.data_ptr() % 16 == 0
        self.inner = self.outer[self.lo:self.lo + n]
        assert self.inner.data_ptr() % 16 == (4 * shift) % 16

    def bands_intact(self):
        return bool((self.outer[:self.lo] == SENTINEL).all()) and bool((self.outer[self.lo + self.n:] == SENTINEL).all())


def _abi_fwd_bwd(N, degree, K, means, center, dc_ptr, dc_stride, rest_ptr, rest_stride, v_col, v_dc_ptr, v_rest_ptr, with_dirs):
    """gspl_sh_fwd + gspl_sh_bwd (origin, +0.5 / clamp) on raw pointers -> colours, v_dirs (or None)."""
    colors = torch.empty(N, 3, dtype=torch.float32, device=DEV)
    clamped = torch.empty(N, 3, dtype=torch.uint8, device=DEV)
    v_dirs = torch.empty(N, 3, dtype=torch.float32, device=DEV) if with_dirs else None
    flags = L.GSPL_SH_ADD_HALF_CLAMP
    L.call("gspl_sh_fwd", N, degree, L.ptr(means), L.ptr(center), dc_ptr, dc_stride, rest_ptr, rest_stride, None, flags,
           L.ptr(colors), L.ptr(clamped), L.stream())
    L.call("gspl_sh_bwd", N, degree, K, L.ptr(means), L.ptr(center), dc_ptr, dc_stride, rest_ptr, rest_stride, None, flags, L.ptr(clamped),
           L.ptr(v_col), 0, v_dc_ptr, v_rest_ptr, L.ptr(v_dirs), L.stream())
    torch.cuda.synchronize()
    return colors, v_dirs


@pytest.mark.parametrize("with_dirs", [True, False], ids=["dirs", "nodirs"])
@pytest.mark.parametrize("merged", [True, False], ids=["merged", "decomposed"])
@pytest.mark.parametrize("N", [1, 257])
@pytest.mark.parametrize("degree", [1, 3])
def test_c_abi_unaligned_outputs_and_padded_strides(degree, N, merged, with_dirs):
    K = (degree + 1) ** 2
    seed = SEEDS[N]
    means, center, dc, rest, w, _ = _inputs(N, K, seed)
    _view_reference(N, K, seed, degree, False)               # (the clamp / fragile shares of these inputs)
    means, center, w = means.to(DEV), center.to(DEV), w.to(DEV)
    cat = torch.cat([dc, rest], 1).to(DEV)
    dcd, restd = dc.to(DEV).contiguous(), rest.to(DEV).contiguous()

    # the dense, aligned run
    if merged:
        v = torch.full((N, 3 * K), SENTINEL, dtype=torch.float32, device=DEV)
        col0, vd0 = _abi_fwd_bwd(N, degree, K, means, center, _p(cat), 3 * K, _p(cat, 3), 3 * K, w, _p(v), _p(v, 3), with_dirs)
        v_dc0, v_rest0 = v[:, :3].clone(), v[:, 3:].clone()
    else:
        v_dc0 = torch.full((N, 3), SENTINEL, dtype=torch.float32, device=DEV)
        v_rest0 = torch.full((N, 3 * (K - 1)), SENTINEL, dtype=torch.float32, device=DEV)
        col0, vd0 = _abi_fwd_bwd(N, degree, K, means, center, _p(dcd), 3, _p(restd), 3 * (K - 1), w, _p(v_dc0), _p(v_rest0), with_dirs)
    assert not bool((v_dc0 == SENTINEL).any()) and not bool((v_rest0 == SENTINEL).any())          # every coefficient of every row is written

    # (a) gradient outputs 4 bytes past 16-byte alignment, between sentinel bands
    if merged:
        out = _Banded(N * 3 * K, shift=1)
        col, vd = _abi_fwd_bwd(N, degree, K, means, center, _p(cat), 3 * K, _p(cat, 3), 3 * K, w, _p(out.inner), _p(out.inner, 3), with_dirs)
        got = out.inner.view(N, 3 * K)
        assert torch.equal(got[:, :3], v_dc0) and torch.equal(got[:, 3:], v_rest0)
        assert out.bands_intact()
    else:
        out_dc, out_rest = _Banded(N * 3, shift=1), _Banded(N * 3 * (K - 1), shift=1)
        col, vd = _abi_fwd_bwd(N, degree, K, means, center, _p(dcd), 3, _p(restd), 3 * (K - 1), w, _p(out_dc.inner), _p(out_rest.inner), with_dirs)
        assert torch.equal(out_dc.inner.view(N, 3), v_dc0) and torch.equal(out_rest.inner.view(N, -1), v_rest0)
        assert out_dc.bands_intact() and out_rest.bands_intact()
    assert torch.equal(col, col0) and (vd0 is None or torch.equal(vd, vd0))

    # (b) row strides larger than the coefficients need: the forward skips the padding, the backward clears it, and nothing past
    # N * stride floats is touched
    if merged:
        stride = 3 * K + 1
        coeffs, out = _Banded(N * stride), _Banded(N * stride)
        coeffs.inner.view(N, stride)[:, :3 * K] = cat.view(N, 3 * K)
        col, vd = _abi_fwd_bwd(N, degree, K, means, center, _p(coeffs.inner), stride, _p(coeffs.inner, 3), stride, w,
                               _p(out.inner), _p(out.inner, 3), with_dirs)
        got = out.inner.view(N, stride)
        assert torch.equal(got[:, :3], v_dc0) and torch.equal(got[:, 3:3 * K], v_rest0)
        assert torch.all(got[:, 3 * K:] == 0), "the backward left the padding columns of a merged row"
        assert torch.all(coeffs.inner.view(N, stride)[:, 3 * K:] == SENTINEL) and torch.equal(coeffs.inner.view(N, stride)[:, :3 * K], cat.view(N, 3 * K))
        assert coeffs.bands_intact() and out.bands_intact()
    else:
        stride = 3 * (K - 1) + 2
        coeffs, out_dc, out = _Banded(N * stride), _Banded(N * 3), _Banded(N * stride)
        coeffs.inner.view(N, stride)[:, :stride - 2] = restd.view(N, -1)
        col, vd = _abi_fwd_bwd(N, degree, K, means, center, _p(dcd), 3, _p(coeffs.inner), stride, w, _p(out_dc.inner), _p(out.inner), with_dirs)
        got = out.inner.view(N, stride)
        assert torch.equal(out_dc.inner.view(N, 3), v_dc0) and torch.equal(got[:, :stride - 2], v_rest0)
        assert torch.all(got[:, stride - 2:] == 0), "the backward left the padding columns of a rest row"
        assert torch.all(coeffs.inner.view(N, stride)[:, stride - 2:] == SENTINEL)
        assert coeffs.bands_intact() and out_dc.bands_intact() and out.bands_intact()
    assert torch.equal(col, col0) and (vd0 is None or torch.equal(vd, vd0))

    # the dense run against fp64 (with the direction gradient: everything the launch produced)
    if with_dirs:
        ref = _view_reference(N, K, seed, degree, False)
        _check_view_against_fp64((col0.cpu(), vd0.cpu(), torch.cat([v_dc0, v_rest0], 1).view(N, K, 3).cpu()), ref, degree, K, "C ABI")

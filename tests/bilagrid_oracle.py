"""fp64 oracle of the bilateral-grid slice and its total-variation loss (include/gspl_hip.h section 14), restated from the maths
with explicit corner gathers (not `grid_sample`): torch autograd gives the gradients.  Runs on any device.

  affine(grids, xy, rgb, idx, w_shift=0)   A [B, H, W, 12]; idx: one grid index per image (ints)
  slice(grids, xy, rgb, idx, w_shift=0)    out [B, H, W, 3]
  slice_grads(grids, xy, rgb, idx, dout)   (out, d grids, d rgb, sum_terms): sum_terms[g, k, z, y, x] = sum over pixels of
                                           |tent weight * dA_k|, the scale of each grid-gradient element's rounding
  tv(x)                                    (1/N) sum_d S_d / K_d

`w_shift` moves the unclamped guidance coordinate w by a small amount: at an integer w (or a clamp bound) the two one-sided
gradients are the slice's at w_shift = +delta and -delta."""
import torch

GRAY = (0.299, 0.587, 0.114)


def _clip(c, size):
    """clamp to [0, size - 1] with grid_sample's border gradient: 0 where clamped AND on the bounds themselves"""
    inside = (c > 0) & (c < size - 1)
    return torch.where(inside, c, c.detach().clamp(0, size - 1))


def affine(grids, xy, rgb, idx, w_shift=0.0, indicator=False):
    """indicator=True: every in-grid corner of the pixel's cell weighs 1 (for `touch` in slice_grads)"""
    N, C, L, GH, GW = grids.shape
    B, H, W, _ = rgb.shape
    xy = xy.expand(B, H, W, 2).to(grids.dtype)
    x, y = xy[..., 0], xy[..., 1]
    gray = GRAY[0] * rgb[..., 0] + GRAY[1] * rgb[..., 1] + GRAY[2] * rgb[..., 2]
    z = 2 * gray - 1
    u = _clip(((2 * x - 1) + 1) / 2 * (GW - 1), GW)
    v = _clip(((2 * y - 1) + 1) / 2 * (GH - 1), GH)
    w = _clip((z + 1) / 2 * (L - 1) + w_shift, L)
    x0, y0, z0 = (t.detach().floor().long() for t in (u, v, w))
    fx, fy, fz = u - x0, v - y0, w - z0
    sel = grids[torch.as_tensor(list(idx), device=grids.device)]            # [B, 12, L, GH, GW]
    flat = sel.reshape(B, 12, -1)
    A = torch.zeros((B, 12, H * W), dtype=grids.dtype, device=grids.device)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cx, cy, cz = x0 + dx, y0 + dy, z0 + dz
                ok = (cx < GW) & (cy < GH) & (cz < L)
                wt = ok.to(grids.dtype) if indicator else (fx if dx else 1 - fx) * (fy if dy else 1 - fy) * (fz if dz else 1 - fz) * ok
                lin = (cz.clamp(max=L - 1) * GH + cy.clamp(max=GH - 1)) * GW + cx.clamp(max=GW - 1)
                vals = torch.gather(flat, 2, lin.reshape(B, 1, -1).expand(B, 12, H * W))
                A = A + vals * wt.reshape(B, 1, -1)
    return A.permute(0, 2, 1).reshape(B, H, W, 12)


def apply_affine(A, rgb):
    M = A.reshape(*A.shape[:-1], 3, 4)
    return (M[..., :3] @ rgb.unsqueeze(-1)).squeeze(-1) + M[..., 3]


def slice(grids, xy, rgb, idx, w_shift=0.0):  # noqa: A001
    return apply_affine(affine(grids, xy, rgb, idx, w_shift), rgb)


def slice_grads(grids, xy, rgb, idx, dout, w_shift=0.0):
    g = grids.detach().double().requires_grad_(True)
    c = rgb.detach().double().requires_grad_(True)
    xyd = xy.detach().double()
    d = dout.detach().double()
    out = slice(g, xyd, c, idx, w_shift)
    dg, dc = torch.autograd.grad((out * d).sum(), (g, c))
    # sum_terms: the same scatter with |dA| (the tent weights are >= 0)
    g2 = grids.detach().double().requires_grad_(True)
    A = affine(g2, xyd, c.detach(), idx, w_shift)
    dA = torch.cat([d.unsqueeze(-1) * c.detach().unsqueeze(-2), d.unsqueeze(-1)], dim=-1).reshape(A.shape)
    terms, = torch.autograd.grad((A * dA.abs()).sum(), (g2,))
    return out.detach(), dg, dc, terms


def touch_terms(grids, xy, rgb, idx, dout):
    """touch[g, k, z, y, x] = sum of |dA_k| over the pixels whose floor cell has the element as a corner: the scale of the change
    that rounding the pixel's coordinates by a few ulps can make to that element (a tent weight moves by the coordinate's error)."""
    g3 = grids.detach().double().requires_grad_(True)
    c = rgb.detach().double()
    d = dout.detach().double()
    A = affine(g3, xy.detach().double(), c, idx, indicator=True)
    dA = torch.cat([d.unsqueeze(-1) * c.unsqueeze(-2), d.unsqueeze(-1)], dim=-1).reshape(A.shape)
    touch, = torch.autograd.grad((A * dA.abs()).sum(), (g3,))
    return touch


def tv(x):
    N, C = x.shape[:2]
    sizes = x.shape[2:]
    total = x.new_zeros(())
    for d, n in enumerate(sizes):
        if n < 2:
            continue
        diff = x.narrow(2 + d, 1, n - 1) - x.narrow(2 + d, 0, n - 1)
        K = C * (n - 1)
        for e, m in enumerate(sizes):
            if e != d:
                K *= m
        total = total + (diff * diff).sum() / K
    return total / N


def tv_grads(x):
    xd = x.detach().double().requires_grad_(True)
    t = tv(xd)
    g, = torch.autograd.grad(t, (xd,))
    return t.detach(), g


def identity_grids(n, gx=16, gy=16, gw=8, dtype=torch.float64):
    ident = torch.tensor([1., 0, 0, 0, 0, 1., 0, 0, 0, 0, 1., 0], dtype=dtype).reshape(1, 12, 1, 1, 1)
    return ident.repeat(n, 1, gw, gy, gx).contiguous()


def meshgrid_xy(H, W, device=None):
    gy, gx = torch.meshgrid(torch.linspace(0, 1., H, device=device), torch.linspace(0, 1., W, device=device), indexing="ij")
    return torch.stack([gx, gy], dim=-1).unsqueeze(0)

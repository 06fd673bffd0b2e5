"""Torch restatement (fp64 by default; the dtype follows the inputs) of include/gspl_hip.h section 15: the depth-to-normal stencil, the
2DGS maps and the surface regulariser sums.  Gradients come from autograd.  Shared by tests/test_normals_shims.py (CPU) and
tests/test_normals_gpu.py; also holds the seeded inputs those tests use."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
EPS = 1e-12


def pixel_rays(A, H, W, normalize_rays=False):
    """r(y, x) = A (x, y, 1)^T, [H, W, 3]; with normalize_rays r / |r|."""
    x, y = torch.meshgrid(torch.arange(W, dtype=A.dtype, device=A.device), torch.arange(H, dtype=A.dtype, device=A.device), indexing="xy")
    r = torch.stack([x, y, torch.ones_like(x)], dim=-1) @ A.T
    return F.normalize(r, dim=-1, eps=EPS) if normalize_rays else r


def points(depth, A, normalize_rays=False):
    H, W = depth.shape
    return depth[..., None] * pixel_rays(A, H, W, normalize_rays)


def depth_to_normal(depth, A, normalize_rays=False, channels_first=False):
    """n = normalize((q(y+1, x) - q(y-1, x)) x (q(y, x+1) - q(y, x-1))) on interior pixels, 0 on the border: [H, W, 3] (or [3, H, W])."""
    if depth.dim() == 3:
        depth = depth[0]
    H, W = depth.shape
    q = points(depth, A.to(depth.dtype), normalize_rays)
    out = torch.zeros_like(q)
    if H >= 3 and W >= 3:
        dx = q[2:, 1:-1] - q[:-2, 1:-1]
        dy = q[1:-1, 2:] - q[1:-1, :-2]
        out[1:-1, 1:-1] = F.normalize(torch.cross(dx, dy, dim=-1), dim=-1, eps=EPS)
    return out.permute(2, 0, 1) if channels_first else out


def forward_bound_terms(depth, A, normalize_rays=False):
    """(S, |c|) [H-2, W-2] of the forward bound |n - n_ref| <= 4 U + kappa U S / |c|:
    S = (|q(y+1,x)| + |q(y-1,x)|) |dy| + (|q(y,x+1)| + |q(y,x-1)|) |dx|."""
    q = points(depth.double(), A.double(), normalize_rays)
    n = lambda v: v.norm(dim=-1)
    dx = q[2:, 1:-1] - q[:-2, 1:-1]
    dy = q[1:-1, 2:] - q[1:-1, :-2]
    S = (n(q[2:, 1:-1]) + n(q[:-2, 1:-1])) * n(dy) + (n(q[1:-1, 2:]) + n(q[1:-1, :-2])) * n(dx)
    return S, n(torch.cross(dx, dy, dim=-1))


def gsplat_rays(camtoworld, K):
    """A of gsplat's `utils.depth_to_points`: pixel centres at +0.5, directions rotated into the world."""
    fx, fy, cx, cy = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    pix = torch.tensor([[1 / fx, 0, (0.5 - cx) / fx], [0, 1 / fy, (0.5 - cy) / fy], [0, 0, 1]], dtype=camtoworld.dtype, device=camtoworld.device)
    return camtoworld[:3, :3] @ pix


def gsplat_depth_to_normal(depths, camtoworlds, Ks, z_depth=True):
    """gsplat's `utils.depth_to_normal` for one image: depths [H, W, 1] -> [H, W, 3]."""
    return depth_to_normal(depths[..., 0], gsplat_rays(camtoworlds, Ks).to(depths.dtype), normalize_rays=not z_depth)


def nan0(x):
    return torch.nan_to_num(x, 0, 0)


def surfel_maps(allmap, normal_rot, A, depth_ratio):
    """(rend_normal [3,H,W], surf_depth [1,H,W], surf_normal [3,H,W]).  The quotient's gradient is routed around torch's 0 / 0: where
    the quotient is not finite the denominator is replaced by 1 first, which leaves planes 0 and 1 with a zero gradient there (the
    header's rule) instead of NaN."""
    alpha = allmap[1:2]
    rend_normal = (allmap[2:5].permute(1, 2, 0) @ normal_rot.to(allmap.dtype).T).permute(2, 0, 1)
    with torch.no_grad():
        ok = torch.isfinite(allmap[0:1] / alpha)
    expected = torch.where(ok, allmap[0:1] / torch.where(ok, alpha, torch.ones_like(alpha)), nan0((allmap[0:1] / alpha).detach()))
    median = nan0(allmap[5:6])
    surf_depth = expected * (1 - depth_ratio) + depth_ratio * median
    surf_normal = depth_to_normal(surf_depth, A, channels_first=True) * alpha.detach()
    return rend_normal, surf_depth, surf_normal


def surface_reg(a, b, dist=None):
    out0 = (1 - (a * b).sum(0)).mean()
    return torch.stack([out0, dist.mean() if dist is not None else torch.zeros_like(out0)])


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------
def quat_to_rot(q):
    w, x, y, z = (float(v) for v in q / q.norm())
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)


def case_depth(H, W, seed):
    """3 + 0.01 x + 0.02 y + 0.3 sin(x / 5) cos(y / 7) + 0.05 rand, plus a +2 step over the lower-right quadrant; fp32 values."""
    g = torch.Generator().manual_seed(seed)
    x, y = torch.meshgrid(torch.arange(W, dtype=torch.float64), torch.arange(H, dtype=torch.float64), indexing="xy")
    d = 3 + 0.01 * x + 0.02 * y + 0.3 * torch.sin(x / 5) * torch.cos(y / 7) + 0.05 * torch.rand(H, W, generator=g, dtype=torch.float64)
    d = d + 2.0 * ((x >= W // 2) & (y >= H // 2)).double()
    return d.float()


def case_focal(H, W):
    return 1600.0 if (H, W) == (1080, 1920) else 170.0


def case_rotation(seed):
    g = torch.Generator().manual_seed(seed + 1000)
    return quat_to_rot(torch.randn(4, generator=g, dtype=torch.float64))


def case_rays(H, W, seed):
    """A = R(random unit quaternion) K^-1, principal point at the centre, f = 170 (1600 at 1080p); fp32 values."""
    f = case_focal(H, W)
    Kinv = torch.tensor([[1 / f, 0, -(W / 2) / f], [0, 1 / f, -(H / 2) / f], [0, 0, 1]], dtype=torch.float64)
    return (case_rotation(seed) @ Kinv).float()



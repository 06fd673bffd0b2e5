"""An fp64 restatement of the reference's `MipSplattingUtils` (internal/models/mip_splatting.py:98-200), pinned to the reference's own
float32 run by tests/golden/ref_mip.npz (tests/test_mip.py) and used as the yardstick of the HIP kernels (tests/test_mip_gpu.py).

filter(means, table)   `compute_3d_filter` over a camera table [C, 16] (R row-major, T, fx, fy, width, height) in float64, plus what a
                       float32 comparison needs: per row the smallest DECISION MARGIN over all cameras (|p.z - 0.01|, absolute, and
                       the four border distances divided by the camera's width or height) and the largest sum of the absolute terms
                       of p.z (the scale of its rounding error).
apply(...)             `apply_3d_filter` / `apply_3d_filter_on_scales`, the reference's expression sqrt(det1 / det2) in float64 under
                       torch autograd (float64 has the range for it: scales of 1e-22 give a det1 of 1e-131), with the exp / sigmoid in
                       front for raw inputs; plus the closed-form magnitudes the error bounds are stated in."""
import numpy as np
import torch

FAR = 100000.0
SQRT_0_2_F32 = float(np.float32(0.2 ** 0.5))      # the reference multiplies a float32 tensor by the Python float: it is rounded first
U = 2.0 ** -24                                    # float32's unit roundoff


def filter(means, table):
    x = np.asarray(means, dtype=np.float64)
    t = np.asarray(table, dtype=np.float64)
    N = x.shape[0]
    distance = np.full(N, FAR)
    valid_any = np.zeros(N, dtype=bool)
    margin = np.full(N, np.inf)
    z_scale = np.zeros(N)
    seen = np.zeros(t.shape[0], dtype=np.int64)
    for c, row in enumerate(t):
        R, T = row[:9].reshape(3, 3), row[9:12]
        fx, fy, w, h = row[12:16]
        p = x @ R.T + T
        z_scale = np.maximum(z_scale, np.abs(x) @ np.abs(R[2]) + abs(T[2]))
        valid_depth = p[:, 2] > 0.01
        z = np.maximum(p[:, 2], 0.001)
        px = p[:, 0] / z * fx + w / 2.0
        py = p[:, 1] / z * fy + h / 2.0
        in_screen = (px >= -0.15 * w) & (px <= 1.15 * w) & (py >= -0.15 * h) & (py <= 1.15 * h)
        valid = valid_depth & in_screen
        distance = np.where(valid, np.minimum(distance, z), distance)
        valid_any |= valid
        seen[c] = valid.sum()
        borders = np.minimum(np.minimum(np.abs(px + 0.15 * w), np.abs(px - 1.15 * w)) / w, np.minimum(np.abs(py + 0.15 * h), np.abs(py - 1.15 * h)) / h)
        margin = np.minimum(margin, np.minimum(np.abs(p[:, 2] - 0.01), borders))
    max_fx = max(float(t[:, 12].max()), 0.0)
    fill = distance[valid_any].max() if valid_any.any() else FAR
    filled = np.where(valid_any, distance, fill)
    return {"distance": distance, "valid_any": valid_any, "filter": filled / max_fx * SQRT_0_2_F32, "margin": margin, "z_scale": z_scale,
            "max_fx": max_fx, "fill": fill, "seen": seen}


def filter_from_parts(distance, valid_any, max_fx):
    """The two final float32 operations of the reference on given float32 distances (torch, any device): what the kernel's second
    launch must reproduce bit for bit."""
    fill = torch.where(valid_any, distance, torch.zeros_like(distance)).max()
    fill = torch.where(valid_any.any(), fill, torch.full_like(fill, FAR))
    return torch.where(valid_any, distance, fill) / max_fx * (0.2 ** 0.5)


def apply(scales, filter_3d, opacities=None, raw_scales=False, raw_opacities=False, compensation=True, v_scales=None, v_second=None):
    """float32 (or float64) arrays -> dict of float64 arrays: scales_out [N, 3], second [N] (o coef | o | coef | None), and with the
    upstream gradients v_scales [N, 3] / v_second [N]: g_scales, g_opacities (of the inputs as given), and the magnitudes
    `mag_scales` (|v_out_i| r_i + |v_coef| prod_{j != i} r_j f^2 / (out_i b_i), times s_i for raw scales), `mag_scales_ref` (the same
    with the reference's two cancelling terms |v_coef| coef (1 / s_i + s_i / b_i) in the second place), and s, o, coef."""
    t = lambda a, g=False: None if a is None else torch.tensor(np.asarray(a, dtype=np.float64).reshape(np.asarray(a).shape[0], -1), requires_grad=g)
    x, f, y = t(scales, True), t(filter_3d), t(opacities, True)
    s = torch.exp(x) if raw_scales else x
    o = None if y is None else (torch.sigmoid(y) if raw_opacities else y)
    scales_square = torch.square(s)
    scales_after_square = scales_square + torch.square(f)
    out = torch.sqrt(scales_after_square)
    coef = torch.sqrt(scales_square.prod(dim=1) / scales_after_square.prod(dim=1))
    if compensation:
        second = coef if o is None else o[:, 0] * coef
    else:
        second = None if o is None else o[:, 0]
    res = {"scales_out": out.detach().numpy(), "second": None if second is None else second.detach().numpy(), "s": s.detach().numpy(),
           "o": None if o is None else o.detach().numpy()[:, 0], "coef": coef.detach().numpy()}
    if v_scales is None and v_second is None:
        return res
    vs = torch.zeros_like(out) if v_scales is None else t(v_scales)
    loss = (out * vs).sum()
    vo = None
    if second is not None and v_second is not None:
        vo = t(v_second)[:, 0]
        loss = loss + (second * vo).sum()
    loss.backward()
    res["g_scales"] = x.grad.numpy()
    res["g_opacities"] = None if y is None else (np.zeros_like(res["o"]) if y.grad is None else y.grad.numpy()[:, 0])
    sd, b, od = s.detach(), scales_after_square.detach(), out.detach()
    r = sd / od
    v_coef = torch.zeros_like(coef.detach()) if (vo is None or not compensation) else (vo if o is None else vo * o.detach()[:, 0])
    others = torch.stack([r[:, 1] * r[:, 2], r[:, 0] * r[:, 2], r[:, 0] * r[:, 1]], dim=1)
    chain = sd if raw_scales else torch.ones_like(sd)
    first = vs.abs() * r
    res["mag_scales"] = ((first + v_coef.abs()[:, None] * others * torch.square(f) / (od * b)) * chain).numpy()
    res["mag_scales_ref"] = ((first + (v_coef.abs() * coef.detach())[:, None] * (1.0 / sd + sd / b)) * chain).numpy()
    res["v_second"] = None if vo is None else vo.numpy()
    return res

"""fp64 restatements of the three SpotLess ops (include/gspl_hip.h section 23), in numpy, from float32 (or float64) inputs.

  resample_matrix(I, O, dtype) -> [O, I]: F.interpolate(mode="bilinear", align_corners=False) of one axis as a matrix.  The indices and
      weights are formed in `dtype` as torch forms them, the source index by one fused multiply-add (float32: what torch does for
      float32 input, checked against F.interpolate itself in tests/test_spotless_cpu.py, and what the kernels do; float64: what torch
      does for float64 input), then used in float64.
  mask(G, A, B, w2, b2, out_size=None, v_out=None, dtype=np.float32) -> a dict with the forward, and with `v_out` every gradient, each
      with the sum of its absolute terms and what the counted bounds of tests/test_spotless.py need (see `mask`).
  error_map(render, gt), robust_mask(err, thr), histogram(err, bins), masked_l1(render, gt, mask, grad=None)
  spot_loss(pred, upper, lower), regulariser(W1, W2), running_stats(hist, counts, bins, percentiles)

The reference's own arithmetic is pinned by tests/golden/ref_spotless.npz (tests/test_spotless_cpu.py)."""
import numpy as np
import torch

HIDDEN = 16
EPS32 = float(np.finfo(np.float32).eps)
Z_ROUNDINGS = 6            # a term of z: product, column combine, row product, row combine, + A, + B
Y_ROUNDINGS = Z_ROUNDINGS + HIDDEN      # ... and at most 16 fmaf of the chain in front of the sigmoid


def resample_axis(I, O, dtype=np.float32):
    """-> i0 [O], i1 [O], l [O], h [O] (weights of i1 and i0, float64 values of `dtype` numbers)."""
    t = np.dtype(dtype).type
    o = np.arange(O).astype(dtype)
    scale = t(I) / t(O)
    # torch's kernels fuse this product and sum (one rounding); in float64 the float32 product and the sum are exact, so rounding the
    # float64 result once IS the float32 fma (for float64 input the difference to a fused sum is below the tests' 1e-12)
    src = (np.float64(scale) * (o + t(0.5)).astype(np.float64) - 0.5).astype(dtype)
    src = np.maximum(src, t(0)).astype(dtype)
    i0 = np.minimum(np.floor(src).astype(np.int64), I - 1)
    i1 = np.minimum(i0 + 1, I - 1)
    l = np.clip((src - i0.astype(dtype)).astype(dtype), t(0), t(1))
    h = (t(1) - l).astype(dtype)
    return i0, i1, l.astype(np.float64), h.astype(np.float64)


def resample_matrix(I, O, dtype=np.float32):
    i0, i1, l, h = resample_axis(I, O, dtype)
    M = np.zeros((O, I), dtype=np.float64)
    np.add.at(M, (np.arange(O), i0), h)
    np.add.at(M, (np.arange(O), i1), l)
    return M


def mask(G, A, B, w2, b2, out_size=None, v_out=None, dtype=np.float32):
    """G [h0, w0, 16], A [mh, 16], B [mw, 16], w2 [16], b2 [1] ->
      out        sigmoid(b2 + w2 . relu(z)) on the mask, or resampled to out_size
      out_bound  the counted float32 bound of `out` (tests/test_spotless.py derives the count)
      z, z_abs   [mh, mw, 16] the hidden pre-activation and the sum of the absolute terms it is made of
      fragile    [mh, mw, 16] |z| <= Z_ROUNDINGS eps32 z_abs: a float32 run may take the other side of the relu
    and with v_out (the shape of `out`), for each of G, A, B, w2, b2:
      v_X        the gradient,   v_X_abs   the sum of its absolute terms,
      v_X_fragile  the sum of the absolute terms of its fragile hidden units, were they active."""
    G, A, B = (np.asarray(a, dtype=np.float64) for a in (G, A, B))
    w2, b2 = np.asarray(w2, dtype=np.float64).reshape(HIDDEN), float(np.asarray(b2, dtype=np.float64).reshape(()))
    (h0, w0, _), mh, mw = G.shape, A.shape[0], B.shape[0]
    Ry, Rx = resample_matrix(h0, mh, dtype), resample_matrix(w0, mw, dtype)
    z = np.einsum("iy,jx,yxc->ijc", Ry, Rx, G) + A[:, None, :] + B[None, :, :]
    z_abs = np.einsum("iy,jx,yxc->ijc", Ry, Rx, np.abs(G)) + np.abs(A)[:, None, :] + np.abs(B)[None, :, :]
    hidden = np.maximum(z, 0.0)
    y = hidden @ w2 + b2
    y_abs = z_abs @ np.abs(w2) + abs(b2)
    y_bound = Y_ROUNDINGS * EPS32 * y_abs
    s = 1.0 / (1.0 + np.exp(-y))
    s_bound = 0.25 * y_bound + 4 * EPS32                      # slope 1/4; expf 2 ulp, 1 + e, 1 / x
    res = {"z": z, "z_abs": z_abs, "fragile": np.abs(z) <= Z_ROUNDINGS * EPS32 * z_abs, "mask": s, "y_abs": y_abs}
    if out_size is None or tuple(out_size) == (mh, mw):
        Sy = Sx = None
        res["out"], res["out_bound"] = s, s_bound
    else:
        Sy, Sx = resample_matrix(mh, out_size[0], dtype), resample_matrix(mw, out_size[1], dtype)
        res["out"] = Sy @ s @ Sx.T
        res["out_bound"] = Sy @ s_bound @ Sx.T + 4 * EPS32   # two products and two combines of values <= 1
    if v_out is None:
        return res
    v_out = np.asarray(v_out, dtype=np.float64)
    v, v_abs = (v_out, np.abs(v_out)) if Sy is None else (Sy.T @ v_out @ Sx, Sy.T @ np.abs(v_out) @ Sx)
    slope = s * (1.0 - s)
    active = (z > 0.0).astype(np.float64)

    def sums(dy, w, gate, unit, tag):
        dz = dy[:, :, None] * w[None, None, :] * gate
        res["v_G" + tag] = np.einsum("iy,jx,ijc->yxc", Ry, Rx, dz)
        res["v_A" + tag] = dz.sum(axis=1)
        res["v_B" + tag] = dz.sum(axis=0)
        res["v_w2" + tag] = np.einsum("ij,ijc->c", dy, unit * gate)
        res["v_b2" + tag] = np.array([dy.sum()])

    fragile = res["fragile"].astype(np.float64)
    sums(v * slope, w2, active, hidden, "")
    sums(v_abs * slope, np.abs(w2), active, z_abs, "_abs")          # (v_w2's term dy relu(z) is made of the terms of z)
    sums(v_abs * slope, np.abs(w2), fragile, np.abs(z), "_fragile")
    res["v_b2_fragile"] = np.zeros(1)                               # dy does not depend on the side of the relu
    return res


def error_map(render, gt):
    d = np.abs(np.asarray(render, dtype=np.float64) - np.asarray(gt, dtype=np.float64))
    return (d[0] + d[1] + d[2]) / 3.0


def robust_mask(err, thr):
    """The reference's `robust_mask` on the per-pixel error [H, W]: inlier = err < thr; 1 where the pixel, or at least 5 of the 9
    pixels of its zero-padded 3 x 3 neighbourhood, are inliers.  (The comparison is made in err's own dtype.)"""
    inl = np.asarray(err) < thr
    pad = np.pad(inl.astype(np.int64), 1)
    H, W = inl.shape
    count = sum(pad[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))
    return (inl | (count >= 5)).astype(np.float32)


def histogram(err, bins):
    """torch.histogram over (0, 1) on the CPU, as `update_running_stats` calls it."""
    return torch.histogram(torch.as_tensor(np.asarray(err, dtype=np.float32)).reshape(-1), bins=bins, range=(0.0, 1.0))[0].numpy()


def masked_l1(render, gt, mask_, grad=None):
    """-> (value, gradient or None): mean(mask[None] |render - gt|) and grad mask sign(render - gt) / (3 H W)."""
    r, g, m = (np.asarray(a, dtype=np.float64) for a in (render, gt, mask_))
    m = m.reshape(r.shape[1:])
    value = float((m[None] * np.abs(r - g)).sum() / r.size)
    return value, (None if grad is None else float(grad) * m[None] * np.sign(r - g) / r.size)


def spot_loss(pred, upper, lower):
    p, u, l = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (pred, upper, lower))
    return float(np.mean(np.maximum(p - u, 0.0) + np.maximum(l - p, 0.0)))


def spot_loss_grad(pred, upper, lower):
    """d spot_loss / d pred, in pred's shape (relu's gradient at 0 is 0)."""
    p = np.asarray(pred, dtype=np.float64)
    u, l = np.asarray(upper, dtype=np.float64).reshape(p.shape), np.asarray(lower, dtype=np.float64).reshape(p.shape)
    return ((p - u > 0).astype(np.float64) - (l - p > 0).astype(np.float64)) / p.size


def regulariser(W1, W2):
    return float(np.abs(W1).max() * np.abs(W2).max())


def running_stats(hist, counts, bins, percentiles):
    """One `update_running_stats` step in float32, as the reference takes it: -> (hist', [edge for each percentile])."""
    hist = (np.float32(0.95) * np.asarray(hist, dtype=np.float32) + np.asarray(counts, dtype=np.float32)).astype(np.float32)
    edges = torch.linspace(0, 1, bins + 1).numpy()
    cum = torch.cumsum(torch.from_numpy(hist), 0).numpy()
    total = torch.sum(torch.from_numpy(hist)).numpy()
    return hist, [edges[np.nonzero(cum >= total * np.float32(q))[0][0]] for q in percentiles]


def fold(state, sf, pe, dtype=np.float64):
    """The fold in numpy: state {'mlp.0.weight', ...}, sf [C, h0, w0], pe = get_positional_encodings(mh, mw, 20) [mh, mw, 80]
    -> G, A, B, w2, b2."""
    W1, b1 = np.asarray(state["mlp.0.weight"], dtype=dtype), np.asarray(state["mlp.0.bias"], dtype=dtype)
    sf = np.asarray(sf, dtype=dtype)
    C = sf.shape[0]
    pe = np.asarray(pe, dtype=dtype)
    G = np.einsum("kc,cyx->yxk", W1[:, :C], sf)
    A = pe[:, 0, :40] @ W1[:, C:C + 40].T + b1
    B = pe[0, :, 40:] @ W1[:, C + 40:].T
    return G, A, B, np.asarray(state["mlp.2.weight"], dtype=dtype).reshape(-1), np.asarray(state["mlp.2.bias"], dtype=dtype)

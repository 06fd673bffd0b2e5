"""fp64 numpy restatement of the Glossy-Gaussian route's view-dependent opacity (include/gspl_hip.h section 25): value, gradient and
the magnitudes the float32 bounds of tests/test_glossy_gpu.py are counted on.  Independent of torch.

    d      = v / max(||v||, 1e-12),  v = means - origin                          (F.normalize)
    raw    = C0 dc + sum_{k = 1}^{(degree + 1)^2 - 1} basis_k(d) rest[:, k - 1] + 0.5      (eval_sh_decomposed + 0.5)
    value  = min(max(raw, 0), 1)
    of sum_n w_n value_n:  v_dc = C0 w [0 <= raw <= 1],  v_rest[:, k - 1] = basis_k(d) w [0 <= raw <= 1],  zero above the degree

tests/test_glossy.py pins this file to the reference's own float64 run (tests/golden/ref_glossy.npz) within 1e-12."""
import numpy as np

EPS32 = 2.0 ** -23
C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)
C4 = (2.5033429417967046, -1.7701307697799304, 0.9461746957575601, -0.6690465435572892, 0.10578554691520431, -0.6690465435572892,
      0.47308734787878004, -1.7701307697799304, 0.6258357354491761)
ORDER = np.repeat(np.arange(5), [1, 3, 5, 7, 9])          # the polynomial degree of basis_k, k = 0 .. 24


def directions(means, origin):
    v = np.asarray(means, dtype=np.float64) - np.asarray(origin, dtype=np.float64).reshape(1, 3)
    return v / np.maximum(np.sqrt((v * v).sum(axis=1, keepdims=True)), 1e-12)


def basis(degree, d, majorant=False):
    """[N, (degree + 1)^2]: the polynomials of `eval_sh_decomposed`, in its forms (so also for a d that is no unit vector).
    majorant: every monomial and every constant replaced by its magnitude, an upper bound of |basis_k| that does not cancel."""
    assert 0 <= degree <= 4
    x, y, z = (np.abs(d[:, i]) if majorant else d[:, i] for i in range(3))
    s = 1.0 if majorant else -1.0                                     # the sign of every subtraction inside a polynomial
    c = (lambda v: abs(v)) if majorant else (lambda v: v)
    b = [np.full(d.shape[0], C0)]
    if degree > 0:
        b += [c(-C1) * y, c(C1) * z, c(-C1) * x]
    if degree > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        b += [c(C2[0]) * xy, c(C2[1]) * yz, c(C2[2]) * (2.0 * zz + s * xx + s * yy), c(C2[3]) * xz, c(C2[4]) * (xx + s * yy)]
    if degree > 2:
        b += [c(C3[0]) * y * (3 * xx + s * yy), c(C3[1]) * xy * z, c(C3[2]) * y * (4 * zz + s * xx + s * yy),
              c(C3[3]) * z * (2 * zz + s * 3 * xx + s * 3 * yy), c(C3[4]) * x * (4 * zz + s * xx + s * yy), c(C3[5]) * z * (xx + s * yy),
              c(C3[6]) * x * (xx + s * 3 * yy)]
    if degree > 3:
        b += [c(C4[0]) * xy * (xx + s * yy), c(C4[1]) * yz * (3 * xx + s * yy), c(C4[2]) * xy * (7 * zz + s * 1), c(C4[3]) * yz * (7 * zz + s * 3),
              c(C4[4]) * (zz * (35 * zz + s * 30) + 3), c(C4[5]) * xz * (7 * zz + s * 3), c(C4[6]) * (xx + s * yy) * (7 * zz + s * 1),
              c(C4[7]) * xz * (xx + s * 3 * yy), c(C4[8]) * (xx * (xx + s * 3 * yy) + s * yy * (3 * xx + s * yy))]
    return np.stack(b, axis=1)


def opacity(degree, means, origin, dc, rest, w=None):
    """means [N, 3], origin [3], dc [N], rest [N, Kr] (Kr >= (degree + 1)^2 - 1; None or [N, 0] at degree 0), w [N] or None ->
    raw, value [N]; with w also v_dc [N], v_rest [N, Kr];
    mag [N] = |C0 dc| + sum_k |basis_k rest_k| + 0.5, and basis [N, K], major [N, K] (the majorant) for the bounds."""
    dc = np.asarray(dc, dtype=np.float64).reshape(-1)
    N, K = dc.shape[0], (degree + 1) ** 2
    rest = np.zeros((N, 0)) if rest is None else np.asarray(rest, dtype=np.float64).reshape(N, -1)
    assert rest.shape[1] >= K - 1
    d = directions(means, origin)
    b, major = basis(degree, d), basis(degree, d, majorant=True)
    used = rest[:, :K - 1]
    raw = C0 * dc + (b[:, 1:] * used).sum(axis=1) + 0.5
    out = {"d": d, "raw": raw, "value": np.minimum(np.maximum(raw, 0.0), 1.0), "basis": b, "major": major,
           "mag": np.abs(C0 * dc) + np.abs(b[:, 1:] * used).sum(axis=1) + 0.5}
    if w is not None:
        g = np.asarray(w, dtype=np.float64).reshape(-1) * ((raw >= 0.0) & (raw <= 1.0))
        out["v_dc"] = C0 * g
        out["v_rest"] = np.zeros_like(rest)
        out["v_rest"][:, :K - 1] = b[:, 1:] * g[:, None]
    return out

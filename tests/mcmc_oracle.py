"""fp64 oracle of the 3DGS-MCMC math (include/gspl_hip.h section 13, csrc/mcmc.hip), restated from the paper and the reference:

  relocation(o, s, n, n_max)        Eq. 9 of Kheradmand et al. straight from the formula, with its condition number
                                    kappa = sum |terms| / |denom| (how much the alternating sum cancels): near 1 for most rows,
                                    but growing with n and o — at o = 1 - 2^-23 about 12 (n = 5), 97 (n = 10), 1.3e3 (n = 20),
                                    2.9e4 (n = 51).  An fp32 evaluation in the written order loses up to ~n^2/2 kappa ulps.
  perturb(means, s, q, o, eps, ...) the reference's `_add_xyz_noise` (internal/density_controllers/mcmc_density_controller.py:93-119,
                                    compute_cov_3d of internal/utils/gaussian_projection.py:211-254) for a given eps
  philox4x32_10 / mcmc_bits / box_muller   the in-kernel generator restated on numpy uint32 words
  reg_fwd / reg_bwd                 `MCMCMetricsModuleMixin.reg_loss` (internal/metrics/mcmc_metrics.py) and its gradients
"""
import math

import numpy as np

U32 = np.uint32
MASK32 = np.uint64(0xFFFFFFFF)


def binoms(n_max: int) -> np.ndarray:
    b = np.zeros((n_max, n_max), dtype=np.float64)
    for n in range(n_max):
        for k in range(n + 1):
            b[n, k] = math.comb(n, k)
    return b


def relocation(opacities, scales, ratios, n_max: int = 51):
    """(new_opacities [M], new_scales [M,3], kappa [M]) in fp64; n = clamp(ratios, 1, n_max)."""
    o = np.asarray(opacities, dtype=np.float64).reshape(-1)
    s = np.asarray(scales, dtype=np.float64).reshape(-1, 3)
    n = np.clip(np.asarray(ratios, dtype=np.int64).reshape(-1), 1, n_max)
    B = binoms(n_max)
    new_o = np.empty_like(o)
    coeff = np.empty_like(o)
    kappa = np.empty_like(o)
    for m in range(o.shape[0]):
        nm = int(n[m])
        x = -math.expm1(math.log1p(-o[m]) / nm) if o[m] < 1 else 1.0
        denom = 0.0
        mag = 0.0
        for i in range(1, nm + 1):
            for k in range(i):
                t = B[i - 1, k] * (-1.0) ** k / math.sqrt(k + 1) * x ** (k + 1)
                denom += t
                mag += abs(t)
        new_o[m] = x
        coeff[m] = o[m] / denom
        kappa[m] = mag / abs(denom)
    return new_o, coeff[:, None] * s, kappa


def rotation_matrix(q):
    q = np.asarray(q, dtype=np.float64)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def activate(scales, rotations, opacities):
    """exp / normalize (F.normalize, eps 1e-12) / sigmoid of the raw parameters, fp64."""
    s = np.exp(np.asarray(scales, dtype=np.float64))
    q = np.asarray(rotations, dtype=np.float64)
    q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)
    o = 1.0 / (1.0 + np.exp(-np.asarray(opacities, dtype=np.float64)))
    return s, q, o


def noise_coefficient(opacities, noise_scale):
    """noise_lr * lr * op_sigmoid(1 - o), op_sigmoid(x) = 1 / (1 + exp(-100 (x - 0.995)))."""
    o = np.asarray(opacities, dtype=np.float64).reshape(-1)
    return noise_scale / (1.0 + np.exp(-100.0 * ((1.0 - o) - 0.995)))


def perturb(means, scales, rotations, opacities, eps, noise_scale, raw: bool):
    """means + c(o) R diag(s^2) R^T eps, fp64 (activated inputs used as given, rotations not normalised: compute_cov_3d)."""
    if raw:
        s, q, o = activate(scales, rotations, opacities)
    else:
        s, q, o = (np.asarray(t, dtype=np.float64) for t in (scales, rotations, opacities))
    s = s.reshape(-1, 3)
    R = rotation_matrix(q.reshape(-1, 4))
    M = R * s[:, None, :]                      # R diag(s)
    cov = M @ M.transpose(0, 2, 1)
    d = np.einsum("nij,nj->ni", cov, np.asarray(eps, dtype=np.float64).reshape(-1, 3))
    return np.asarray(means, dtype=np.float64).reshape(-1, 3) + noise_coefficient(o, noise_scale)[:, None] * d


# ---- Philox4x32-10 + Box-Muller ----------------------------------------------------------------------------------------------------
def _mulhilo(a, b):
    p = a.astype(np.uint64) * np.uint64(b)
    return (p >> np.uint64(32)).astype(U32), (p & MASK32).astype(U32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Salmon et al. (SC'11) on uint32 arrays: 10 rounds, key schedule W = (0x9E3779B9, 0xBB67AE85)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=U32).copy() for c in (c0, c1, c2, c3))
    k0, k1 = U32(k0), U32(k1)
    with np.errstate(over="ignore"):
        for r in range(10):
            hi0, lo0 = _mulhilo(c0, 0xD2511F53)
            hi1, lo1 = _mulhilo(c2, 0xCD9E8D57)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
            if r < 9:
                k0 = U32((int(k0) + 0x9E3779B9) & 0xFFFFFFFF)
                k1 = U32((int(k1) + 0xBB67AE85) & 0xFFFFFFFF)
    return np.stack([c0, c1, c2, c3], axis=1)


def mcmc_bits(n: int, seed: int, offset: int, first: int = 0) -> np.ndarray:
    """u32 [n,4]: Gaussian i draws counter (lo(offset / 4), hi(offset / 4), lo(i), hi(i)) under key (lo(seed), hi(seed)) — the first
    block of curand_init(seed, subsequence = i, offset), offset a multiple of 4."""
    assert offset % 4 == 0
    i = np.arange(first, first + n, dtype=np.uint64)
    blk = offset >> 2
    c0 = np.full(n, blk & 0xFFFFFFFF, dtype=U32)
    c1 = np.full(n, (blk >> 32) & 0xFFFFFFFF, dtype=U32)
    c2, c3 = (i & MASK32).astype(U32), (i >> np.uint64(32)).astype(U32)
    return philox4x32_10(c0, c1, c2, c3, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def uniforms(bits) -> np.ndarray:
    """u = ((b >> 8) + 1) 2^-24 in (0, 1]."""
    return ((np.asarray(bits, dtype=np.uint64) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24


def box_muller(bits) -> np.ndarray:
    u = uniforms(bits)
    r01 = np.sqrt(-2.0 * np.log(u[:, 0]))
    r23 = np.sqrt(-2.0 * np.log(u[:, 2]))
    return np.stack([r01 * np.cos(2 * np.pi * u[:, 1]), r01 * np.sin(2 * np.pi * u[:, 1]), r23 * np.cos(2 * np.pi * u[:, 3])], axis=1)


# ---- regulariser ---------------------------------------------------------------------------------------------------------------------
def reg_fwd(opacities, scales, opacity_w, scale_w, raw: bool):
    o = np.asarray(opacities, dtype=np.float64).reshape(-1)
    s = np.asarray(scales, dtype=np.float64).reshape(-1)
    fo = 1.0 / (1.0 + np.exp(-o)) if raw else o
    gs = np.exp(s) if raw else s
    return opacity_w * np.abs(fo).mean(), scale_w * np.abs(gs).mean()


def reg_bwd(opacities, scales, opacity_w, scale_w, raw: bool, g_o: float = 1.0, g_s: float = 1.0):
    o = np.asarray(opacities, dtype=np.float64)
    s = np.asarray(scales, dtype=np.float64)
    N = o.size
    if raw:
        sg = 1.0 / (1.0 + np.exp(-o))
        return g_o * opacity_w / N * sg * (1 - sg), g_s * scale_w / (3 * N) * np.exp(s)
    return g_o * opacity_w / N * np.sign(o), g_s * scale_w / (3 * N) * np.sign(s)

"""fp64 / integer oracle of the Taming-3DGS scoring arithmetic (numpy only; restates
internal/density_controllers/taming_3dgs_density_controller.py `Taming3DGSUtils.normalize`, the aggregate of `compute_gaussian_score`,
`get_edges` and the min-max normalisation of `on_train_start`).  Pinned to the reference and to PIL by tests/golden/ref_taming.npz
(tests/test_taming.py); the ops of gspl_amd.ops.taming are pinned to it."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32


def as_float32(row):
    """A row as the ops read it: float32 as it is, int32 through float(x)."""
    row = np.asarray(row)
    return row.astype(np.float32) if row.dtype != np.float32 else row


def valid(row):
    """> 0 and not NaN, on the float32 bit pattern: sign clear, non-zero, at most +inf's."""
    bits = as_float32(row).view(np.uint32)
    return (bits > 0) & (bits <= 0x7f800000)


def positive_median(row):
    """-> (n, the valid entry of rank (n - 1) // 2 in ascending order as float32; NaN when n == 0), by sorting."""
    v = as_float32(row)
    v = np.sort(v[valid(row)])
    n = int(v.size)
    return n, (v[(n - 1) // 2] if n else np.float32(np.nan))


def positive_medians(rows):
    out = [positive_median(r) for r in rows]
    return np.array([n for n, _ in out], dtype=np.int32), np.array([m for _, m in out], dtype=np.float32)


def score(rows, coeffs, medians, w, visible, counts=None):
    """fp64: w * (sum_r coeffs[r] * rows[r] / medians[r] over the valid entries) * visible, with `medians` as given (the kernel's own
    where the test isolates the aggregate).  coeffs are rounded to float32 first, as both sides receive them.  Also returns the sum of
    the terms' magnitudes under the same weights, the scale of the error bound when coefficients differ in sign."""
    total = np.zeros(len(rows[0]), dtype=np.float64)
    mag = np.zeros_like(total)
    for r, row in enumerate(rows):
        if counts is not None and counts[r] == 0:
            continue
        ok = valid(row)
        v = as_float32(row).astype(np.float64)
        with np.errstate(all="ignore"):
            t = np.where(ok, np.float64(np.float32(coeffs[r])) * (v / np.float64(medians[r])), 0.0)
        total += t
        mag += np.abs(t)
    vis = np.asarray(visible).astype(np.float64)
    return np.float64(w) * total * vis, abs(np.float64(w)) * mag * vis


def quantise(image):
    """[3, H, W] uint8, or float32 in [0, 1] as ToPILImage takes it: x * 255 in float32, truncated to a byte."""
    image = np.asarray(image)
    if image.dtype == np.uint8:
        return image.astype(np.int64)
    return np.trunc(image.astype(np.float32) * np.float32(255.0)).astype(np.int64)


def grey(image):
    """PIL's L conversion: (R 19595 + G 38470 + B 7471 + 0x8000) >> 16."""
    c = quantise(image)
    return (c[0] * 19595 + c[1] * 38470 + c[2] * 7471 + 0x8000) >> 16


def edge_bytes(image):
    """PIL's FIND_EDGES of the grey image, in integers: 8 centre - neighbours clipped to 0 .. 255; the one-pixel border unfiltered."""
    g = grey(image)
    e = g.copy()
    H, W = g.shape
    for y in range(1, H - 1):
        for x in range(1, W - 1):
            e[y, x] = min(max(9 * g[y, x] - g[y - 1:y + 2, x - 1:x + 2].sum(), 0), 255)
    return e


def edge_bytes_fast(image):
    """The same by slices (for the larger test images)."""
    g = grey(image)
    e = g.copy()
    H, W = g.shape
    if H >= 3 and W >= 3:
        around = sum(g[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
        e[1:-1, 1:-1] = np.clip(9 * g[1:-1, 1:-1] - around, 0, 255)
    return e


def normalised_edges(e):
    """fp64: (e / 255 - min) / (max - min) from the integer edge values; NaN throughout for a constant image."""
    x = e.astype(np.float64) / 255.0
    with np.errstate(all="ignore"):
        return (x - x.min()) / (x.max() - x.min())


def loss_map(render, gt, mse_importance, edge_importance, edges):
    """fp64 `get_loss_map`: the channel mean of |render - gt|, min-max normalised, times mse_importance, plus edge_importance * edges."""
    l1 = np.abs(render.astype(np.float64) - gt.astype(np.float64)).mean(axis=0)
    with np.errstate(all="ignore"):
        l1n = (l1 - l1.min()) / (l1.max() - l1.min())
    return mse_importance * l1n + edge_importance * edges.astype(np.float64)


def count_array(start_count, multiplier, densify_until_iter, densify_from_iter, densification_interval, mode):
    """`get_count_array` (Eq. 2 of the paper) in Python floats and its int() truncations."""
    budget = int(start_count * float(multiplier)) if mode == "multiplier" else multiplier
    num_steps = (densify_until_iter + densification_interval - 1) // densification_interval - densify_from_iter // densification_interval
    increasable = max(budget - start_count, 0)
    k = 2 * (increasable / num_steps)
    a = (increasable - k * num_steps) / (num_steps * num_steps)
    return [int(1 * a * (x ** 2) + (k * x) + start_count) for x in range(num_steps)]

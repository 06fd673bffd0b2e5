"""fp64 numpy oracle of the grid encoding of include/gspl_hip.h section 20, written from the rules and sharing no code with the
package: the level table, the forward, and the backward with, per table entry, the count of contributions and the sum of their
magnitudes (what the tolerances of tests/test_hashgrid.py are made of)."""
import math
from collections import namedtuple

import numpy as np

PRIMES = (1, 2654435761, 805459861)
U = 2.0 ** -24          # half an ulp of 1 in float32
Levels = namedtuple("Levels", "D F scales resolutions sizes offsets hashed total")
Result = namedtuple("Result", "out out_abs v_table v_table_count v_table_abs v_x v_x_abs")


def levels(D, n_levels, F, log2_hashmap_size, base_resolution, per_level_scale, dense=False):
    scales, resolutions, sizes, hashed = [], [], [], []
    for level in range(n_levels):
        scale = np.float32(2.0 ** (level * math.log2(per_level_scale)) * base_resolution - 1.0)
        res = int(math.ceil(float(scale))) + 1
        size = (min(res ** D, (2 ** 32 - 1) // 2) + 7) // 8 * 8
        if not dense:
            size = min(size, 2 ** log2_hashmap_size)
        scales.append(scale)
        resolutions.append(res)
        sizes.append(size)
        hashed.append(res ** D > size)
    offsets = [sum(sizes[:level]) for level in range(n_levels)]
    return Levels(D, F, scales, resolutions, sizes, offsets, hashed, sum(sizes))


def positions(x, scale):
    """x [N, D] float32 -> (cell [N, D] as uint32 values in int64, frac [N, D] float64); pos = float32(x * scale + 0.5), one rounding
    (the product of two float32 is exact in double)."""
    pos = (x.astype(np.float64) * np.float64(scale) + 0.5).astype(np.float32)
    floor = np.floor(pos)
    cell = np.clip(floor.astype(np.float64), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64) & 0xFFFFFFFF
    return cell, (pos - floor).astype(np.float64)


def corner_rows(lv, level, cell, corner):
    D, res, size = lv.D, lv.resolutions[level], lv.sizes[level]
    index = np.zeros(cell.shape[0], dtype=np.int64)
    for d in range(D):
        c = (cell[:, d] + ((corner >> d) & 1)) & 0xFFFFFFFF
        if lv.hashed[level]:
            index ^= (c * PRIMES[d]) & 0xFFFFFFFF
        else:
            index = (index + c * (res ** d & 0xFFFFFFFF)) & 0xFFFFFFFF
    return index % size


def min_frac_margin(x, lv):
    """Per point, the smallest distance of any level's frac to 0 or 1 (the input construction of the random tests drops small ones)."""
    margin = np.full(x.shape[0], 1.0)
    for level in range(len(lv.scales)):
        _, frac = positions(x, lv.scales[level])
        margin = np.minimum(margin, np.minimum(frac, 1 - frac).min(axis=1))
    return margin


def encode(x, table, lv, v_out=None, want_x=False):
    """x [N, D] float32, table [total, F] -> Result.  out_abs = sum |w t|; with v_out [N, L F]: v_table, the count of contributions per
    table entry, v_table_abs = sum |w g|; with want_x: v_x and v_x_abs = sum_l scale_l sum_corners |other weights| sum_f |t g|."""
    x = np.asarray(x, dtype=np.float32)
    table = np.asarray(table, dtype=np.float64).reshape(lv.total, lv.F)
    N, D, F, L = x.shape[0], lv.D, lv.F, len(lv.scales)
    out, out_abs = np.zeros((N, L * F)), np.zeros((N, L * F))
    v_table = count = v_table_abs = v_x = v_x_abs = None
    if v_out is not None:
        v_out = np.asarray(v_out, dtype=np.float64)
        v_table, v_table_abs = np.zeros((lv.total, F)), np.zeros((lv.total, F))
        count = np.zeros((lv.total, F), dtype=np.int64)
        if want_x:
            v_x, v_x_abs = np.zeros((N, D)), np.zeros((N, D))
    for level in range(L):
        cell, frac = positions(x, lv.scales[level])
        g = None if v_out is None else v_out[:, level * F:(level + 1) * F]
        for corner in range(1 << D):
            factors = [frac[:, d] if (corner >> d) & 1 else 1 - frac[:, d] for d in range(D)]
            w = np.prod(factors, axis=0)
            rows = lv.offsets[level] + corner_rows(lv, level, cell, corner)
            t = table[rows]
            out[:, level * F:(level + 1) * F] += w[:, None] * t
            out_abs[:, level * F:(level + 1) * F] += np.abs(w[:, None] * t)
            if g is None:
                continue
            live = (g != 0).any(axis=1)          # a (point, level) whose gradient is all zero contributes nothing
            np.add.at(v_table, rows[live], w[live, None] * g[live])
            np.add.at(v_table_abs, rows[live], np.abs(w[live, None] * g[live]))
            np.add.at(count, rows[live], 1)
            if want_x:
                dot, dot_abs = (t * g).sum(axis=1), np.abs(t * g).sum(axis=1)
                for d in range(D):
                    other = np.prod([factors[e] for e in range(D) if e != d], axis=0) if D > 1 else np.ones(N)
                    sign = 1.0 if (corner >> d) & 1 else -1.0
                    v_x[:, d] += np.float64(lv.scales[level]) * sign * other * dot
                    v_x_abs[:, d] += np.float64(lv.scales[level]) * other * dot_abs
    return Result(out, out_abs, v_table, count, v_table_abs, v_x, v_x_abs)

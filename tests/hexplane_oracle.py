"""numpy oracle of the HexPlane field of include/gspl_hip.h section 22, written from the rules and sharing no code with the package:
the layout, the packing, the forward, and both gradients with the counts and sums of magnitudes that the tolerances of
tests/test_hexplane.py are made of.

The pixel coordinates are computed in float32, one rounded operation after the other in the documented order (what the reference's
float32 run does, and what the kernels do): kernel and oracle take the same cell for every input.  Everything after them —
interpolation, the product over the planes, the gradients — is float64.  `encode(..., double=True)` computes the coordinates in float64
too: that is the reference's `HexPlaneField.double()`, which tests/golden/ref_hexplane.npz records."""
import itertools
from collections import namedtuple

import numpy as np

U = 2.0 ** -24          # half an ulp of 1 in float32
PLANES = list(itertools.combinations(range(4), 2))
Layout = namedtuple("Layout", "F resolutions planes total")
Result = namedtuple("Result", "out out_abs v_table v_table_count v_table_abs v_x v_x_abs")


def layout(resolution, multires, F):
    """planes[l][p] = (a, b, R_a, R_b, first row); the multiplier applies to the spatial axes only."""
    resolutions, planes, at = [], [], 0
    for m in multires:
        res = [int(r) * int(m) for r in resolution[:3]] + [int(resolution[3])]
        resolutions.append(res)
        row = []
        for a, b in PLANES:
            row.append((a, b, res[a], res[b], at))
            at += res[a] * res[b]
        planes.append(row)
    return Layout(int(F), resolutions, planes, at)


def pack(grids, lay):
    """grids[l][p] [1, F, R_b, R_a] -> table [total, F]: texel (i_b, i_a) of a plane is row first + i_b R_a + i_a."""
    table = np.zeros((lay.total, lay.F))
    for level, row in enumerate(lay.planes):
        for p, (a, b, Ra, Rb, first) in enumerate(row):
            g = np.asarray(grids[level][p], dtype=np.float64)
            assert g.shape == (1, lay.F, Rb, Ra), (g.shape, (1, lay.F, Rb, Ra))
            table[first:first + Ra * Rb] = g[0].transpose(1, 2, 0).reshape(Ra * Rb, lay.F)
    return table


def coordinates(x, t, aabb, double=False):
    """p [N, 4] = ((x - aabb[0]) (2 / (aabb[1] - aabb[0])) - 1, t) in float32 (or float64), and the scale [3] as float64."""
    ft = np.float64 if double else np.float32
    x, aabb = np.asarray(x, dtype=ft), np.asarray(aabb, dtype=ft)
    t = np.broadcast_to(np.asarray(t, dtype=ft).reshape(-1), (x.shape[0],))
    scale = ft(2.0) / (aabb[1] - aabb[0])
    xn = (x - aabb[0]) * scale - ft(1.0)
    p = np.concatenate([xn, t[:, None]], axis=1)
    assert p.dtype == ft
    return p, scale.astype(np.float64)


def pixels(c, R):
    """c [N] -> (i0 [N] int, f [N] float64, inside [N] bool): i = ((c + 1) / 2) (R - 1) clamped to [0, R - 1], in c's own precision."""
    ft = c.dtype.type
    raw = ((c + ft(1.0)) / ft(2.0)) * ft(R - 1)
    i = np.minimum(np.maximum(raw, ft(0.0)), ft(R - 1))
    assert i.dtype == c.dtype
    i0 = np.floor(i)
    return i0.astype(np.int64), (i - i0).astype(np.float64), (raw > 0) & (raw < R - 1)


def encode(x, t, table, aabb, lay, v_out=None, want_x=False, double=False):
    """x [N, 3], t a number or [N], table [total, F], aabb [2, 3] -> Result.
    out_abs = product over the planes of A_p, A_p = sum over the corners of |w v|.
    With v_out [N, L F]: v_table; per table entry the count of contributions (corners that ARE texels, of (point, level) blocks whose
    gradient is not all zero) and v_table_abs = sum |w g prod_{q != p} I_q|.
    With want_x: v_x and v_x_abs = sum over levels, channels, planes holding the axis and corners of |pixels per unit g w_other v
    prod_{q != p} I_q|."""
    table = np.asarray(table, dtype=np.float64).reshape(lay.total, lay.F)
    p4, scale = coordinates(x, t, aabb, double)
    N, F, L = p4.shape[0], lay.F, len(lay.planes)
    out, out_abs = np.zeros((N, L * F)), np.zeros((N, L * F))
    v_table = count = v_table_abs = v_x = v_x_abs = None
    if v_out is not None:
        v_out = np.asarray(v_out, dtype=np.float64)
        v_table, v_table_abs = np.zeros((lay.total, F)), np.zeros((lay.total, F))
        count = np.zeros((lay.total, F), dtype=np.int64)
        if want_x:
            v_x, v_x_abs = np.zeros((N, 3)), np.zeros((N, 3))
    for level in range(L):
        res = lay.resolutions[level]
        axes = [pixels(p4[:, d], res[d]) for d in range(4)]
        interp, mags, corners = [], [], []
        for a, b, Ra, Rb, first in lay.planes[level]:
            (ia, fa, _), (ib, fb, _) = axes[a], axes[b]
            I, A, cs = np.zeros((N, F)), np.zeros((N, F)), []
            for sb in (0, 1):
                for sa in (0, 1):
                    ja, jb = ia + sa, ib + sb
                    texel = (ja < Ra) & (jb < Rb)          # a corner with index R contributes nothing
                    wa, wb = (fa if sa else 1 - fa), (fb if sb else 1 - fb)
                    rows = first + np.minimum(jb, Rb - 1) * Ra + np.minimum(ja, Ra - 1)
                    v = np.where(texel[:, None], table[rows], 0.0)
                    I += (wa * wb)[:, None] * v
                    A += np.abs((wa * wb)[:, None] * v)
                    cs.append((sa, sb, wa, wb, rows, texel, v))
            interp.append(I)
            mags.append(A)
            corners.append(cs)
        sl = slice(level * F, (level + 1) * F)
        out[:, sl] = np.prod(interp, axis=0)
        out_abs[:, sl] = np.prod(mags, axis=0)
        if v_out is None:
            continue
        g = v_out[:, sl]
        live = (g != 0).any(axis=1)
        for p, (a, b, Ra, Rb, first) in enumerate(lay.planes[level]):
            other = np.prod([interp[q] for q in range(6) if q != p], axis=0)
            for sa, sb, wa, wb, rows, texel, v in corners[p]:
                m = live & texel
                term = (wa * wb)[:, None] * g * other
                np.add.at(v_table, rows[m], term[m])
                np.add.at(v_table_abs, rows[m], np.abs(term[m]))
                np.add.at(count, rows[m], 1)
                if not want_x:
                    continue
                for d, sign, w_other in ((a, 1.0 if sa else -1.0, wb), (b, 1.0 if sb else -1.0, wa)):
                    if d == 3:
                        continue
                    per_unit = np.where(axes[d][2], (res[d] - 1) / 2.0 * scale[d], 0.0)
                    v_x[:, d] += per_unit * sign * w_other * (v * g * other).sum(axis=1)
                    v_x_abs[:, d] += np.abs(per_unit) * w_other * np.abs(v * g * other).sum(axis=1)
    return Result(out, out_abs, v_table, count, v_table_abs, v_x, v_x_abs)

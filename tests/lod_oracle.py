"""The partition-LoD route's per-frame front in numpy float64 (nothing here reads the reference tree): the distances and the level rule of
internal/renderers/partition_lod_renderer.py:498-503, 553-557, the frustum of lines 564-588, the separating-axis visibility test of
include/gspl_hip.h section 26, `dst_start`, the gather as a concatenation of slices, and an INDEPENDENT visibility criterion: the
Chebyshev radius of the intersection of the two solids' 12 half-spaces by linear programming (the interior is non-empty iff it is > 0).

tests/golden/ref_lod.npz (made by tests/golden/make_lod_golden.py from the reference's own `get_partition_distances` in float64) pins
`distances`; the linear programme pins `separation`'s sign (tests/test_lod.py)."""
import numpy as np

NEAR, FAR_FACTOR, DEGENERATE = 0.1, 10.0, 1e-12
FACES = ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7))
EDGES = ((0, 1), (1, 2), (0, 4), (1, 5), (2, 6), (3, 7))


def distances(camera_center, transform, box_min, box_max):
    """sqrt(sum(clamp(max(min - p, p - max), 0)^2)),  p = (c @ T)[:2]  -> [P]"""
    p = (np.asarray(camera_center, np.float64) @ np.asarray(transform, np.float64))[:2]
    dxy = np.maximum(np.asarray(box_min, np.float64) - p, p - np.asarray(box_max, np.float64))
    return np.sqrt((np.maximum(dxy, 0.0) ** 2).sum(-1))


def levels(distance, thresholds, n_levels):
    """The reference fills with -1 (which indexes the coarsest level) and walks the thresholds from the coarsest down, so the finest
    level whose threshold the distance is below wins: the smallest i with distance < thresholds[i], else L - 1."""
    lod = np.full(distance.shape, n_levels - 1, np.int64)
    for i in range(n_levels - 2, -1, -1):
        lod[distance < thresholds[i]] = i
    return lod


def threshold_margin(distance, thresholds):
    """min_i |distance - thresholds[i]| per partition (inf without thresholds)."""
    if len(thresholds) == 0:
        return np.full(distance.shape, np.inf)
    return np.abs(distance[:, None] - np.asarray(thresholds, np.float64)[None]).min(-1)


def frustum(fx, fy, cx, cy, width, height, far, near=NEAR):
    """[8, 3]: the image corners (0, 0), (W, 0), (W, H), (0, H) through K^-1, at depth `near` and then at depth `far`."""
    uv = np.array([[0.0, 0.0], [width, 0.0], [width, height], [0.0, height]])
    rays = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(4)], -1)
    return np.concatenate([rays * near, rays * far], 0)


def to_camera(corners, world_to_camera):
    """The reference's transposed matrix: x_cam = x_world @ M[:3, :3] + M[3, :3]."""
    M = np.asarray(world_to_camera, np.float64)
    return np.asarray(corners, np.float64) @ M[:3, :3] + M[3, :3]


def _axes(A, B):
    for V in (A, B):
        for a, b, c, d in FACES:
            u, v = V[..., c, :] - V[..., a, :], V[..., d, :] - V[..., b, :]
            yield np.cross(u, v), (u * u).sum(-1) * (v * v).sum(-1)
    for i, j in EDGES:
        a = A[..., j, :] - A[..., i, :]
        for k, m in EDGES:
            b = B[..., m, :] - B[..., k, :]
            yield np.cross(a, b), (a * a).sum(-1) * (b * b).sum(-1)


def separation(A, B):
    """The largest gap, over the 6 + 6 face normals and the 6 x 6 edge cross products, between the shadows of the convex hexahedra A and
    B [..., 8, 3] (broadcast against each other) on the axis, in units of length (-inf when every axis is degenerate).  >= 0: some axis
    separates them."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    sep = np.full(np.broadcast_shapes(A.shape[:-2], B.shape[:-2]), -np.inf)
    for n, scale in _axes(A, B):
        n2 = (n * n).sum(-1)
        valid = n2 > DEGENERATE * scale
        a, b = (A * n[..., None, :]).sum(-1), (B * n[..., None, :]).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            gap = np.maximum(a.min(-1) - b.max(-1), b.min(-1) - a.max(-1)) / np.sqrt(n2)
        sep = np.where(valid, np.maximum(sep, gap), sep)
    return sep if sep.ndim else float(sep)


def visibility(distance, corners, world_to_camera, fx, fy, cx, cy, width, height):
    """-> (visible [P] bool, separation [P]): no separating axis with a non-negative gap; the nearest partition (the lowest index among
    equals) always."""
    F = frustum(fx, fy, cx, cy, width, height, FAR_FACTOR * distance.max())
    cam = to_camera(corners, world_to_camera)
    sep = separation(F, cam)
    visible = sep < 0
    visible[int(np.argmin(distance))] = True
    return visible, sep


def dst_start(lod, visible, seg_start, n_partitions):
    """[P + 1]: the exclusive scan of the chosen segments' lengths, an invisible partition counting 0."""
    seg_start = np.asarray(seg_start, np.int64)
    index = np.asarray(lod, np.int64) * n_partitions + np.arange(n_partitions)
    lengths = np.where(visible, seg_start[index + 1] - seg_start[index], 0)
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def gather(array, lod, visible, seg_start, n_partitions):
    """The chosen segments of a flat array, in partition order, as a concatenation of slices."""
    parts = [array[seg_start[l * n_partitions + p]:seg_start[l * n_partitions + p + 1]] for p, l in enumerate(lod) if visible[p]]
    return np.concatenate(parts, 0) if parts else array[:0]


# ---- the independent criterion ------------------------------------------------------------------------------------------------------
def half_spaces(V):
    """A convex hexahedron's 6 faces as n . x <= c with unit n pointing outwards."""
    centre = V.mean(0)
    out = []
    for a, b, c, d in FACES:
        n = np.cross(V[c] - V[a], V[d] - V[b])
        n = n / np.linalg.norm(n)
        offset = n @ V[[a, b, c, d]].mean(0)
        if n @ centre > offset:
            n, offset = -n, -offset
        out.append((n, offset))
    return out


def chebyshev_radius(A, B):
    """The radius of the largest ball inside both solids (<= 0: their interiors do not meet): maximise r subject to
    n_i . x + r <= c_i over the 12 faces."""
    from scipy.optimize import linprog
    planes = half_spaces(A) + half_spaces(B)
    A_ub = np.array([np.append(n, 1.0) for n, _ in planes])
    b_ub = np.array([c for _, c in planes])
    res = linprog(c=[0, 0, 0, -1.0], A_ub=A_ub, b_ub=b_ub, bounds=[(None, None)] * 4, method="highs")
    assert res.status == 0, res.message
    return float(res.x[3])


def random_box(rng):
    """The case law of tests/test_lod.py: side lengths uniform in [0.5, 6], a corner uniform in [-12, 12]^3, a random rotation about the
    box's own centre and a shift in [-3, 3]^3.  Corners in the reference's order: the top face clockwise, then the bottom face."""
    size = rng.uniform(0.5, 6.0, 3)
    origin = rng.uniform(-12.0, 12.0, 3)
    ring = np.array([[0, 0], [0, 1], [1, 1], [1, 0]], np.float64)
    unit = np.concatenate([np.concatenate([ring, np.ones((4, 1))], 1), np.concatenate([ring, np.zeros((4, 1))], 1)], 0)
    corners = origin + unit * size
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    centre = corners.mean(0)
    return (corners - centre) @ Rm.T + centre + rng.uniform(-3.0, 3.0, 3)

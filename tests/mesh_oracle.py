"""fp64 restatements of the mesh-extraction route (include/gspl_hip.h section 18), written fresh from the published algorithms:
the running-average TSDF fusion of 2DGS's `extract_mesh_unbounded` (Huang et al., 2D Gaussian Splatting) and marching tetrahedra on the
Kuhn decomposition.  PARITY WITH THE REFERENCE'S OWN MODULE IS UNPINNED: internal/utils/gs2d_mesh_utils.py imports open3d, trimesh
and skimage at module level and cannot be imported where these tests run; these oracles pin this implementation to the algorithm as
the header states it.  Also here: the analytic test scene, the fp32/fp64 torch restatement of the reference's formulation (used to
measure KAPPA on the CPU, and by tools/mesh_extract_time.py as the baseline) and a small mesh toolbox (components, Euler
characteristic, signed volume)."""
import itertools
import math

import numpy as np
import torch

U = 2.0 ** -24
FLAG = 64 * U


# ---- the scene ----------------------------------------------------------------------------------------------------------------------------
def orbit_cameras(V, H, W, radius=2.2, tan_half=0.4):
    """V cameras on an orbit of `radius` around the origin with varying elevation, looking at the origin.  Returns
    (full_projection [V,4,4] float32, row-vector convention with p.w = camera z; world_to_camera [V,4,4] float32 row-vector; a list of
    (R, t, tanx, tany) in fp64 for the analytic maps)."""
    full, w2cs, geo = [], [], []
    tanx, tany = tan_half, tan_half * (H / W if W >= H else 1.0) if min(H, W) > 1 else tan_half
    for v in range(V):
        az = 2 * math.pi * (v + 0.25) / V
        el = 0.5 * math.sin(1.7 * v + 0.3)
        eye = radius * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])            # world -> camera, x right, y down, z forward
        t = -R @ eye
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = R, t
        zn, zf = 0.01, 100.0
        P = np.zeros((4, 4))
        P[0, 0], P[1, 1], P[2, 2], P[2, 3], P[3, 2] = 1 / tanx, 1 / tany, zf / (zf - zn), -zf * zn / (zf - zn), 1.0
        full.append((P @ w2c).T)
        w2cs.append(w2c.T)
        geo.append((R, t, tanx, tany))
    return np.stack(full).astype(np.float32), np.stack(w2cs).astype(np.float32), geo


def sphere_maps(geo, H, W, sphere_radius=0.5, perturb=0.01):
    """depth [V,H,W] float32: the analytic z-depth of the sphere |x| = sphere_radius through every pixel centre (align_corners=True:
    pixel 0 at -1, pixel W-1 at +1; a single pixel at 0), plus perturb sin(x/3) cos(y/4) on the sphere, 0 off it; rgb [V,3,H,W]: a smooth
    pattern on the sphere, 0 off it."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    nx = xs / (W - 1) * 2 - 1 if W > 1 else np.zeros_like(xs)
    ny = ys / (H - 1) * 2 - 1 if H > 1 else np.zeros_like(ys)
    depth, rgb = [], []
    for R, t, tanx, tany in geo:
        eye = -R.T @ t
        d = np.stack([nx * tanx, ny * tany, np.ones_like(nx)], -1) @ R          # world directions with camera z = 1
        a, b, c = (d * d).sum(-1), 2 * (d @ eye), eye @ eye - sphere_radius ** 2
        disc = b * b - 4 * a * c
        hit = disc > 0
        s = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a), 0.0)
        depth.append(np.where(hit, s + perturb * np.sin(xs / 3) * np.cos(ys / 4), 0.0))
        rgb.append(np.stack([np.where(hit, 0.5 + 0.45 * np.sin(0.21 * xs + ch) * np.cos(0.17 * ys - ch), 0.0) for ch in range(3)]))
    return np.stack(depth).astype(np.float32), np.stack(rgb).astype(np.float32)


def contract_np(x):
    mag = np.linalg.norm(x, axis=-1, keepdims=True)
    return np.where(mag < 1, x, (2 - 1 / np.maximum(mag, 1e-300)) * (x / np.maximum(mag, 1e-300)))


def uncontract_np(y):
    mag = np.linalg.norm(y, axis=-1, keepdims=True)
    safe = np.maximum(mag, 1e-300)
    return np.where(mag < 1, y, (1 / (2 - mag)) * (y / safe))


def scene_points(M, contract, center, radius, seed, sphere_radius=0.5):
    """M samples as float32: 60 % within +-0.15 of the sphere surface, the rest uniform in radius up to 2.5 (world space); contracted
    around (center, radius) when `contract` is on."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(M, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    near = rng.random(M) < 0.6
    r = np.where(near, sphere_radius + rng.uniform(-0.15, 0.15, M), rng.uniform(0.0, 2.5, M))
    x = d * r[:, None]
    if contract:
        x = contract_np((x - np.asarray(center)) / radius)
    return x.astype(np.float32)


# ---- fusion, fp64 ---------------------------------------------------------------------------------------------------------------------------
def lattice_points(lo, hi, n, block=None):
    """The header's lattice in float32 (the step rounded, then one fused multiply-add): [M,3], k fastest."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    b, m = ((0, 0, 0), n) if block is None else block
    axes = []
    for a in range(3):
        g = (np.arange(m[a]) + b[a]).astype(np.float32)
        if n[a] > 1:
            step = np.float32(np.float32(hi[a] - lo[a]) / np.float32(n[a] - 1))
            # one rounding, as a fused multiply-add: the product of two floats is exact in fp64
            axes.append((np.float64(lo[a]) + g.astype(np.float64) * np.float64(step)).astype(np.float32))
        else:
            axes.append(np.full(m[a], lo[a], np.float32))
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def _spread_maps(maps, own=False):
    """maps [C,H,W] -> [H', W'] (H' = max(H-1, 1)): per 2x2 tap cell the largest max - min over the channels (`own`: that), then the
    largest of the 3x3 cell neighbourhood."""
    C, H, W = maps.shape
    y0, x0 = np.arange(max(H - 1, 1)), np.arange(max(W - 1, 1))
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    taps = np.stack([maps[:, y0][:, :, x0], maps[:, y0][:, :, x1], maps[:, y1][:, :, x0], maps[:, y1][:, :, x1]])
    cell = (taps.max(0) - taps.min(0)).max(0)
    if own:
        return cell
    pad = np.pad(cell, 1, mode="edge")
    return np.max([pad[dy:dy + cell.shape[0], dx:dx + cell.shape[1]] for dy in range(3) for dx in range(3)], axis=0)


def fuse(samples, views, depth, rgb=None, center=(0, 0, 0), radius=1.0, voxel_size=1.0, sdf_trunc=None, depth_trunc=None, contract=False,
         state=None):
    """The header's gspl_tsdf_fuse in fp64 on the float32 inputs.  Returns a dict: tsdf, weight [M], color [M,3] (or None), and for the
    tests flagged [M] (some discrete decision of some view within 64 U of flipping), s_tsdf [M] (max over the counted views of
    S_v / T) and s_rgb [M] (max of |c| + G_rgb)."""
    s = np.asarray(samples, np.float32).astype(np.float64)
    M = s.shape[0]
    views = np.asarray(views, np.float32).astype(np.float64).reshape(-1, 4, 4)
    depth = np.asarray(depth, np.float32).astype(np.float64)
    V, H, W = depth.shape
    with_rgb = rgb is not None
    if with_rgb:
        rgb = np.asarray(rgb, np.float32).astype(np.float64)
    base = float(np.float32(sdf_trunc)) if sdf_trunc is not None and sdf_trunc > 0 else 5.0 * float(np.float32(voxel_size))
    T = np.full(M, base)
    x = s
    if contract:
        mag = np.linalg.norm(s, axis=-1)
        T = np.where(mag > 1, T * (1 / (2 - np.minimum(mag, 1.9))), T)
        x = uncontract_np(s) * float(np.float32(radius)) + np.asarray(center, np.float32).astype(np.float64)
    cut = float(np.float32(depth_trunc)) if depth_trunc is not None and depth_trunc > 0 else None
    if state is None:
        tsdf, weight, color = np.ones(M, np.float32), np.ones(M, np.float32), np.zeros((M, 3), np.float32) if with_rgb else None
    else:
        tsdf, weight = state[0].astype(np.float32).copy(), state[1].astype(np.float32).copy()
        color = state[2].astype(np.float32).copy() if with_rgb else None
    tsdf, weight = tsdf.astype(np.float64), weight.astype(np.float64)
    color = color.astype(np.float64) if with_rgb else None
    flagged, s_tsdf, s_rgb = np.zeros(M, bool), np.zeros(M), np.zeros(M)
    xh = np.concatenate([x, np.ones((M, 1))], -1)
    with np.errstate(all="ignore"):
        for v in range(V):
            p = xh @ views[v]
            mags = np.abs(xh) @ np.abs(views[v])
            z = p[:, 3]
            pix = p[:, :2] / z[:, None]
            proj = (pix > -1).all(-1) & (pix < 1).all(-1) & (z > 0)
            near = (np.abs(np.abs(p[:, 0]) - np.abs(z)) <= FLAG * (mags[:, 0] + mags[:, 3])) \
                | (np.abs(np.abs(p[:, 1]) - np.abs(z)) <= FLAG * (mags[:, 1] + mags[:, 3])) | (np.abs(z) <= FLAG * mags[:, 3])
            near |= ~np.isfinite(pix).all(-1)
            ix = np.clip((np.nan_to_num(pix[:, 0]) + 1) / 2 * (W - 1), 0, W - 1)
            iy = np.clip((np.nan_to_num(pix[:, 1]) + 1) / 2 * (H - 1), 0, H - 1)
            x0, y0 = np.clip(np.floor(ix).astype(int), 0, W - 1), np.clip(np.floor(iy).astype(int), 0, H - 1)
            x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
            fx, fy = ix - x0, iy - y0
            wts = ((1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy)

            def tap(m):
                return m[y0, x0] * wts[0] + m[y0, x1] * wts[1] + m[y1, x0] * wts[2] + m[y1, x1] * wts[3]
            d = tap(depth[v])
            cy, cx = np.minimum(y0, max(H - 2, 0)), np.minimum(x0, max(W - 2, 0))
            scale = ((W - 1) + (H - 1)) * mags[:, 3] / np.abs(z)
            G = scale * _spread_maps(depth[v][None])[cy, cx]
            S = np.abs(d) + mags[:, 3] + G
            sdf = d - z
            near_cut = proj & (np.abs(sdf + T) <= FLAG * S)
            ok = proj & (sdf > -T)
            if cut is not None:
                # d > 0: four taps that are all exactly 0 give exactly 0 in any precision, so next to a depth edge the decision is
                # fragile only where the sample's own cell holds the edge, or where its pixel lies within rounding of the cell's border
                G_own = scale * _spread_maps(depth[v][None], own=True)[cy, cx]
                border = (np.minimum(np.minimum(fx, 1 - fx), np.minimum(fy, 1 - fy)) <= FLAG * scale) & (G > 0)
                near_zero = ((np.abs(d) <= FLAG * (np.abs(d) + G_own)) & (np.abs(d) + G_own > 0)) | border
                near_cut |= proj & ((np.abs(d - cut) <= FLAG * (np.abs(d) + G)) | near_zero)
                ok &= (d > 0) & (d <= cut)
            flagged |= near | near_cut
            val = np.clip(sdf / T, -1, 1)
            w = weight
            tsdf = np.where(ok, (tsdf * w + np.where(ok, val, 0.0)) / (w + 1), tsdf)
            s_tsdf = np.where(ok, np.maximum(s_tsdf, np.where(ok, S / T, 0.0)), s_tsdf)
            if with_rgb:
                c = np.stack([tap(rgb[v, ch]) for ch in range(3)], -1)
                color = np.where(ok[:, None], (color * w[:, None] + np.where(ok[:, None], c, 0.0)) / (w[:, None] + 1), color)
                Gc = scale * _spread_maps(rgb[v])[cy, cx]
                s_rgb = np.where(ok, np.maximum(s_rgb, np.where(ok, np.abs(c).max(-1) + Gc, 0.0)), s_rgb)
            weight = np.where(ok, w + 1, w)
    return {"tsdf": tsdf, "weight": weight, "color": color, "flagged": flagged, "s_tsdf": s_tsdf, "s_rgb": s_rgb}


def fuse_torch(samples, views, depth, rgb=None, center=None, radius=1.0, voxel_size=1.0, contract=False, state=None):
    """The reference's formulation (`compute_unbounded_tsdf` + `compute_sdf_perframe`) restated with torch ops in the dtype and on the
    device of `samples`: per view a matrix product, a division, two `grid_sample` calls and masked updates.  Returns (tsdf, weight, color)."""
    import torch.nn.functional as F
    if contract:
        mag = torch.linalg.norm(samples, dim=-1)
        trunc = 5 * voxel_size * torch.ones_like(samples[:, 0])
        mask = mag > 1
        trunc[mask] *= 1 / (2 - mag[mask].clamp(max=1.9))
        m = mag[..., None]
        samples = torch.where(m < 1, samples, (1 / (2 - m)) * (samples / m)) * radius + center
    else:
        trunc = 5 * voxel_size
    if state is None:
        tsdfs, weights = torch.ones_like(samples[:, 0]), torch.ones_like(samples[:, 0])
        rgbs = torch.zeros((samples.shape[0], 3), dtype=samples.dtype, device=samples.device)
    else:
        tsdfs, weights, rgbs = state
    homo = torch.cat([samples, torch.ones_like(samples[..., :1])], dim=-1)
    for v in range(depth.shape[0]):
        new = homo @ views[v]
        z = new[..., -1:]
        pix = new[..., :2] / new[..., -1:]
        mask = ((pix > -1.) & (pix < 1.) & (z > 0)).all(dim=-1)
        sampled = F.grid_sample(depth[v][None, None], pix[None, None], mode="bilinear", padding_mode="border", align_corners=True).reshape(-1, 1)
        sdf = (sampled - z).flatten()
        mask = mask & (sdf > -trunc)
        val = torch.clamp(sdf / trunc, min=-1.0, max=1.0)[mask]
        w = weights[mask]
        wp = w + 1
        tsdfs[mask] = (tsdfs[mask] * w + val) / wp
        if rgb is not None:
            col = F.grid_sample(rgb[v][None], pix[None, None], mode="bilinear", padding_mode="border", align_corners=True).reshape(3, -1).T
            rgbs[mask] = (rgbs[mask] * w[:, None] + col[mask]) / wp[:, None]
        weights[mask] = wp
    return tsdfs, weights, rgbs


# ---- marching tetrahedra ------------------------------------------------------------------------------------------------------------------
_OFF = np.array([[(m >> 2) & 1, (m >> 1) & 1, m & 1] for m in range(8)])
_BIT = (4, 2, 1)
TETS = [(0, _BIT[a], _BIT[a] | _BIT[b], 7) for a, b, c in itertools.permutations((0, 1, 2))]      # lexicographic
_DIRECTION = {(1, 0, 0): 0, (0, 1, 0): 1, (0, 0, 1): 2, (1, 1, 0): 3, (1, 0, 1): 4, (0, 1, 1): 5, (1, 1, 1): 6}
_EDGES = {1: [((0, 1), (0, 2), (0, 3))], 3: [((0, 3), (1, 3), (2, 3))], 2: [((0, 2), (0, 3), (1, 3)), ((0, 2), (1, 3), (1, 2))]}


def _tet_cases(tet):
    """For one tetrahedron: {inside bits: [triangles]}, a triangle = three (corner mask A, corner mask B) with A the lower node, already
    oriented (normal from the inside corners to the outside ones; the test at the edge midpoints, which decides it for every crossing)."""
    cases = {}
    for bits in range(1, 15):
        inside = [t for t in range(4) if (bits >> t) & 1]
        outside = [t for t in range(4) if not (bits >> t) & 1]
        names = inside + outside
        cin = np.mean([_OFF[tet[t]] for t in inside], axis=0)
        cout = np.mean([_OFF[tet[t]] for t in outside], axis=0)
        tris = []
        for tri in _EDGES[len(inside)]:
            edges = []
            for a, b in tri:
                ta, tb = sorted((names[a], names[b]))
                edges.append((tet[ta], tet[tb]))
            mid = [(_OFF[a] + _OFF[b]) / 2.0 for a, b in edges]
            if np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), cin - cout) > 0:
                edges = [edges[0], edges[2], edges[1]]
            tris.append(edges)
        cases[bits] = tris
    return cases


_CASES = [_tet_cases(tet) for tet in TETS]


def marching_tetrahedra(volume, level, origin, step, global_dims=None, block_offset=None):
    """The header's marching tetrahedra on a float32 volume, positions in fp64 from the float32 origin / step.  Returns a dict:
    counts [(X-1)(Y-1)(Z-1)] (triangles per cell), vertices [3T,3] fp64, keys [3T] int64, and per vertex the quantities of the test's
    bound: pa, pb [3T,3] (the edge's end nodes), fa, fb [3T]."""
    vol = np.asarray(volume, np.float32)
    X, Y, Z = vol.shape
    G = tuple(vol.shape) if global_dims is None else tuple(global_dims)
    b = (0, 0, 0) if block_offset is None else tuple(block_offset)
    origin = np.asarray(origin, np.float32).astype(np.float64)
    step = np.asarray(step, np.float32).astype(np.float64)
    level32 = np.float32(level)
    empty = {"counts": np.zeros(max(X - 1, 0) * max(Y - 1, 0) * max(Z - 1, 0), np.int64), "vertices": np.zeros((0, 3)), "keys": np.zeros(0, np.int64),
             "pa": np.zeros((0, 3)), "pb": np.zeros((0, 3)), "fa": np.zeros(0), "fb": np.zeros(0)}
    if min(X, Y, Z) < 2:
        return empty
    ci, cj, ck = [a.reshape(-1) for a in np.meshgrid(np.arange(X - 1), np.arange(Y - 1), np.arange(Z - 1), indexing="ij")]
    corner = np.stack([vol[ci + o[0], cj + o[1], ck + o[2]] for o in _OFF], -1)           # [cells, 8]
    inside = corner < level32
    counts = np.zeros(ci.shape[0], np.int64)
    order, rec = [], []
    for q, tet in enumerate(TETS):
        bits = sum(inside[:, tet[t]].astype(np.int64) << t for t in range(4))
        for pattern, tris in _CASES[q].items():
            cells = np.nonzero(bits == pattern)[0]
            if cells.size == 0:
                continue
            counts[cells] += len(tris)
            for n, tri in enumerate(tris):
                for e, (ma, mb) in enumerate(tri):
                    order.append((cells * 12 + q * 2 + n) * 3 + e)
                    ga = np.stack([ci[cells] + b[0], cj[cells] + b[1], ck[cells] + b[2]], -1) + _OFF[ma]
                    d = tuple(int(t) for t in (_OFF[mb] - _OFF[ma]))
                    key = ((ga[:, 0] * G[1] + ga[:, 1]) * G[2] + ga[:, 2]).astype(np.int64) * 8 + _DIRECTION[d]
                    fa, fb = corner[cells, ma].astype(np.float64), corner[cells, mb].astype(np.float64)
                    pa, pb = origin + ga * step, origin + (ga + np.array(d)) * step
                    t = (float(level32) - fa) / (fb - fa)
                    rec.append((key, pa + t[:, None] * (pb - pa), pa, pb, fa, fb))
    if not order:
        return empty
    perm = np.argsort(np.concatenate(order), kind="stable")
    cat = lambda i: np.concatenate([r[i] for r in rec])[perm]
    return {"counts": counts, "keys": cat(0), "vertices": cat(1), "pa": cat(2), "pb": cat(3), "fa": cat(4), "fb": cat(5)}


def index_soup(vertices, keys):
    """(vertices [Nv,3], faces [T,3], keys [Nv]): triangles' vertices merged by key, keys ascending."""
    unique, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    return vertices[first], inverse.reshape(-1, 3), unique


# ---- a small mesh toolbox ----------------------------------------------------------------------------------------------------------------
def edge_table(faces):
    """(directed edges [3T,2], undirected edge id per face edge [T,3], number of undirected edges)."""
    f = np.asarray(faces).reshape(-1, 3)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und = np.sort(directed, axis=1)
    _, ids = np.unique(und, axis=0, return_inverse=True)
    ids = ids.reshape(-1)
    return directed, ids.reshape(3, -1).T, int(ids.max()) + 1 if ids.size else 0


def is_closed_oriented(faces):
    """Every undirected edge in exactly two faces and no directed edge twice."""
    directed, ids, n = edge_table(faces)
    if n == 0:
        return True
    return bool((np.bincount(ids.reshape(-1), minlength=n) == 2).all()) and np.unique(directed, axis=0).shape[0] == directed.shape[0]


def euler(n_vertices, faces):
    _, _, n_edges = edge_table(faces)
    return n_vertices - n_edges + np.asarray(faces).reshape(-1, 3).shape[0]


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces).reshape(-1, 3)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def components(faces):
    """A label per face (faces connected through shared edges), labels 0.. ordered by size descending; and the sizes."""
    f = np.asarray(faces).reshape(-1, 3)
    T = f.shape[0]
    _, ids, n = edge_table(f)
    labels = np.arange(T)
    while True:
        low = np.full(n, T)
        np.minimum.at(low, ids.reshape(-1), np.repeat(labels, 3))
        new = np.minimum(labels, low[ids].min(1))
        new = new[new]
        if np.array_equal(new, labels):
            break
        labels = new
    roots, inverse, sizes = np.unique(labels, return_inverse=True, return_counts=True)
    rank = np.argsort(-sizes, kind="stable")
    relabel = np.empty_like(rank)
    relabel[rank] = np.arange(rank.size)
    return relabel[inverse.reshape(-1)], sizes[rank]


def sphere_volume(n, radius=0.5, origin=(-0.8, -0.7, -0.75), step=None):
    """An n^3 float32 volume of |p| - radius on a lattice with a non-zero origin; returns (volume, origin, step)."""
    origin = np.asarray(origin, np.float32)
    step = (np.full(3, 1.6 / (n - 1)) if step is None else np.asarray(step)).astype(np.float32)
    axes = [origin[a].astype(np.float64) + np.arange(n) * float(step[a]) for a in range(3)]
    p = np.stack(np.meshgrid(*axes, indexing="ij"), -1)
    return (np.linalg.norm(p, axis=-1) - radius).astype(np.float32), origin, step


def torus_volume(n=24, R=0.5, r=0.2):
    """A torus around the z axis on an ANISOTROPIC lattice; returns (volume, origin, step)."""
    origin = np.array([-0.9, -0.95, -0.4], np.float32)
    step = np.array([1.8 / (n - 1), 1.9 / (n - 1), 0.8 / (n - 1)], np.float32)
    axes = [origin[a].astype(np.float64) + np.arange(n) * float(step[a]) for a in range(3)]
    p = np.stack(np.meshgrid(*axes, indexing="ij"), -1)
    return (np.sqrt((np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - R) ** 2 + p[..., 2] ** 2) - r).astype(np.float32), origin, step


def extract(views, depth, lo, hi, n, level=0.0, **fuse_args):
    """The fp64 pipeline: fuse on the float32 lattice, marching tetrahedra, merge.  Returns (vertices, faces) in lattice space."""
    pts = lattice_points(lo, hi, n)
    vol = fuse(pts, views, depth, **fuse_args)["tsdf"].astype(np.float32).reshape(n)
    lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    step = np.array([np.float32(np.float32(hi32[a] - lo32[a]) / np.float32(max(n[a] - 1, 1))) for a in range(3)], np.float32)
    out = marching_tetrahedra(vol, level, lo32, step)
    v, f, _ = index_soup(out["vertices"], out["keys"])
    return v, f

"""The mesh-extraction kernels on the GPU (include/gspl_hip.h section 18) against the fp64 restatements of tests/mesh_oracle.py, and the
public pipeline of gspl_amd.mesh end to end on an analytic scene.  Parity with the reference's own module is UNPINNED (it imports
open3d, trimesh and skimage and cannot be imported here); the oracles pin the algorithm as the header states it.

Fusion.  The oracle flags a sample when in any view a discrete decision (|pix| = 1, z = 0, d - z = -sdf_trunc, the depth_trunc cut)
lies within 64 U (U = 2^-24) of flipping, scaled by the magnitudes involved; at most 2 % of a case may be flagged, every unflagged sample
has exactly the oracle's weight and  |tsdf - ref| <= KAPPA U (max_v S_v / sdf_trunc + 4),  S_v = |d| + sum_j |x_j||P_j4| + G_v,
G_v = ((W-1) + (H-1)) spread sum_j |x_j||P_j4| / |z|  (spread: the largest max - min of a 2x2 tap cell in the 3x3 cell neighbourhood
of the sample's pixel); colour likewise with the rgb taps' spread and no 1 / sdf_trunc.
KAPPA: the reference's formulation restated with float32 torch ops (mesh_oracle.fuse_torch) on the CPU, over the cases of this file and
four larger ones (up to 20 000 samples, 16 views, 128x176), needs kappa <= 0.349 for tsdf and <= 0.165 for colour against this
oracle, with at most 0.40 % of a case flagged and no unflagged weight mismatch (re-measured with the committed oracle; the issue's
own measurement was 0.42).  The kernel gets 4x that, rounded up to a power of two: KAPPA = 2 either way.

Marching tetrahedra.  Same float32 volume on both sides: counts per cell and keys exactly equal (the decisions compare identical fp32
numbers), every vertex within  |p_B - p_A| 8 U (|level| + |f_A| + |f_B|) / |f_B - f_A| + 4 U max(|p_A|, |p_B|)."""
import functools
import math
import types

import numpy as np
import pytest
import torch

import mesh_oracle as MO

pytestmark = pytest.mark.gpu

U = MO.U
KAPPA = 2.0
CENTER, RADIUS, VOXEL = (0.03, -0.02, 0.01), 1.0, 2.0 / 64

# (M, V, H, W, contract, with_rgb): every value of every parameter at least once
FUSE_CASES = [
    (1, 1, 1, 1, False, False),
    (63, 3, 2, 3, True, True),
    (64, 7, 5, 67, False, True),
    (65, 3, 37, 50, True, False),
    (4099, 7, 37, 50, True, True),
    (4099, 7, 37, 50, False, False),
    (4099, 1, 5, 67, True, False),
    (65, 7, 1, 1, False, True),
]


def _dev():
    import gspl_amd  # noqa: F401
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _scene(V, H, W):
    full, w2c, geo = MO.orbit_cameras(V, H, W)
    depth, rgb = MO.sphere_maps(geo, H, W)
    return full, w2c, depth, rgb


@functools.lru_cache(maxsize=None)
def _case(M, V, H, W, contract, with_rgb):
    full, _, depth, rgb = _scene(V, H, W)
    pts = MO.scene_points(M, contract, CENTER, RADIUS, seed=M + 7 * V)
    ref = MO.fuse(pts, full, depth, rgb if with_rgb else None, center=CENTER, radius=RADIUS, voxel_size=VOXEL, contract=contract)
    return pts, full, depth, rgb, ref


def _gpu_fuse(pts, full, depth, rgb, contract, with_rgb, splits, dev, **table_args):
    from gspl_amd import ops
    state = ops.tsdf_init(pts.shape[0], with_rgb, dev)
    table = ops.tsdf_table(CENTER, RADIUS, VOXEL, contract=contract, with_rgb=with_rgb, device=dev, **table_args)
    P, D, C = torch.from_numpy(full).to(dev), torch.from_numpy(depth).to(dev), torch.from_numpy(rgb).to(dev)
    X = torch.from_numpy(pts).to(dev)
    for a, b in splits:
        ops.tsdf_fuse(state, table, P[a:b], D[a:b], C[a:b] if with_rgb else None, points=X)
    return state


def _check_against_oracle(state, ref, with_rgb, label):
    tsdf, weight = state[0].cpu().numpy().astype(np.float64), state[1].cpu().numpy().astype(np.float64)
    firm = ~ref["flagged"]
    share = float(ref["flagged"].mean())
    wrong = int((weight[firm] != ref["weight"][firm]).sum())
    err = np.abs(tsdf - ref["tsdf"])
    bound = KAPPA * U * (ref["s_tsdf"] + 4)
    worst = float((err[firm] / (U * (ref["s_tsdf"][firm] + 4))).max()) if firm.any() else 0.0
    print(f"{label}: flagged {share:.4%}, unflagged weight mismatches {wrong}, tsdf kappa {worst:.3f}")
    assert share <= 0.02, f"{label}: {share:.3%} of the samples flagged (cap 2 %)"
    assert wrong == 0, f"{label}: {wrong} unflagged samples differ from the oracle's weight"
    assert (err[firm] <= bound[firm]).all(), f"{label}: tsdf kappa {worst:.3f} > {KAPPA}"
    if with_rgb:
        cerr = np.abs(state[2].cpu().numpy().astype(np.float64) - ref["color"]).max(-1)
        cworst = float((cerr[firm] / (U * (ref["s_rgb"][firm] + 4))).max()) if firm.any() else 0.0
        print(f"{label}: colour kappa {cworst:.3f}")
        assert (cerr[firm] <= KAPPA * U * (ref["s_rgb"][firm] + 4)).all(), f"{label}: colour kappa {cworst:.3f} > {KAPPA}"
    else:
        assert state[2] is None


@pytest.mark.parametrize("M, V, H, W, contract, with_rgb", FUSE_CASES)
def test_fusion_against_the_oracle(M, V, H, W, contract, with_rgb):
    dev = _dev()
    pts, full, depth, rgb, ref = _case(M, V, H, W, contract, with_rgb)
    if M == 4099 and V >= 7 and H >= 37 and W >= 50:
        live = float(((ref["weight"] > 2) & (np.abs(ref["tsdf"]) < 1)).mean())
        assert live >= 0.25, f"vacuous case: only {live:.2%} of the samples fuse at least two views inside the band"
    splits = [(0, 2), (2, 7)] if V == 7 else [(0, V)]          # 2 + 5, the state carried
    state = _gpu_fuse(pts, full, depth, rgb, contract, with_rgb, splits, dev)
    _check_against_oracle(state, ref, with_rgb, f"M={M} V={V} {H}x{W} contract={contract} rgb={with_rgb}")


def test_depth_trunc_and_sdf_trunc_against_the_oracle():
    """The bounded mode's two table entries: an explicit sdf_trunc and the depth_trunc cut (here between the sphere's near and far depths)."""
    dev = _dev()
    M, V, H, W = 4099, 3, 37, 50
    full, _, depth, rgb = _scene(V, H, W)
    pts = MO.scene_points(M, False, CENTER, RADIUS, seed=5)
    ref = MO.fuse(pts, full, depth, rgb, voxel_size=VOXEL, sdf_trunc=0.11, depth_trunc=1.9)
    plain = MO.fuse(pts, full, depth, rgb, voxel_size=VOXEL)
    assert (ref["weight"] != plain["weight"]).mean() > 0.05          # the two entries change what counts
    state = _gpu_fuse(pts, full, depth, rgb, False, True, [(0, V)], dev, sdf_trunc=0.11, depth_trunc=1.9)
    _check_against_oracle(state, ref, True, "sdf_trunc=0.11 depth_trunc=1.9")


def test_two_calls_give_the_bits_of_one_and_runs_repeat():
    dev = _dev()
    pts, full, depth, rgb, _ = _case(4099, 7, 37, 50, True, True)
    one = _gpu_fuse(pts, full, depth, rgb, True, True, [(0, 7)], dev)
    again = _gpu_fuse(pts, full, depth, rgb, True, True, [(0, 7)], dev)
    two = _gpu_fuse(pts, full, depth, rgb, True, True, [(0, 2), (2, 7)], dev)
    three = _gpu_fuse(pts, full, depth, rgb, True, True, [(0, 1), (1, 6), (6, 7)], dev)
    for a, b, c, d in zip(one, again, two, three):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
    assert float((one[1] > 1).float().mean()) > 0.3


@pytest.mark.parametrize("n", [(1, 1, 1), (2, 3, 5), (17, 9, 4)])
def test_lattice_mode_is_the_explicit_points_of_the_headers_formula(n):
    from gspl_amd import ops
    dev = _dev()
    full, _, depth, rgb = _scene(3, 37, 50)
    lo, hi = (-0.62, -0.55, -0.7), (0.58, 0.66, 0.61)
    P, D, C = (torch.from_numpy(a).to(dev) for a in (full, depth, rgb))
    blocks = [None] if n != (17, 9, 4) else [None, ((1, 2, 1), (9, 4, 3)), ((16, 8, 3), (1, 1, 1))]
    for block in blocks:
        pts = MO.lattice_points(lo, hi, n, block)
        M = pts.shape[0]
        table = ops.tsdf_table(CENTER, RADIUS, VOXEL, contract=False, with_rgb=True, lo=lo, hi=hi, device=dev)
        explicit = ops.tsdf_fuse(ops.tsdf_init(M, True, dev), table, P, D, C, points=torch.from_numpy(pts).to(dev))
        lattice = ops.tsdf_fuse(ops.tsdf_init(M, True, dev), table, P, D, C, lattice=n, block=block)
        for a, b in zip(explicit, lattice):
            assert torch.equal(a, b), f"lattice {n} block {block}"
        if n == (17, 9, 4) and block is None:
            assert float((lattice[1] > 1).float().mean()) > 0.2


def test_nothing_to_fuse_leaves_the_state_untouched():
    from gspl_amd import _lib as L, ops
    dev = _dev()
    full, _, depth, _ = _scene(3, 2, 3)
    P, D = torch.from_numpy(full).to(dev), torch.from_numpy(depth).to(dev)
    table = ops.tsdf_table(CENTER, RADIUS, VOXEL, device=dev)
    state = (torch.full((5,), 0.25, device=dev), torch.full((5,), 3.0, device=dev), None)
    pts = torch.zeros(5, 3, device=dev)
    ops.tsdf_fuse(state, table, P[:0], D[:0], points=pts)                                        # V == 0
    assert torch.equal(state[0], torch.full((5,), 0.25, device=dev)) and torch.equal(state[1], torch.full((5,), 3.0, device=dev))
    empty = ops.tsdf_init(0, False, dev)
    ops.tsdf_fuse(empty, table, P, D, points=torch.zeros(0, 3, device=dev))                      # M == 0
    assert empty[0].numel() == 0
    fn = L.lib().gspl_tsdf_fuse
    assert fn(0, None, 0, 0, 0, 0, 0, 0, 0, 0, 0, None, 3, 2, 3, None, None, None, None, None, None, None) == 0
    assert fn(5, None, 0, 0, 0, 0, 0, 0, 0, 0, 0, None, 0, 2, 3, None, None, None, None, None, None, None) == 0


# ---- marching tetrahedra ------------------------------------------------------------------------------------------------------------------
def _mtet_both(vol, level, origin, step, **kw):
    from gspl_amd import ops
    dev = _dev()
    ref = MO.marching_tetrahedra(vol, level, origin, step, kw.get("global_dims"), kw.get("block_offset"))
    v, k = ops.marching_tetrahedra_soup(torch.from_numpy(vol).to(dev), level, origin.tolist(), step.tolist(), **kw)
    return ref, v.cpu().numpy(), k.cpu().numpy()


def _check_soup(ref, v, k, level, label):
    assert k.shape[0] == ref["keys"].shape[0] == 3 * int(ref["counts"].sum()), f"{label}: {k.shape[0] // 3} triangles, the oracle has {ref['counts'].sum()}"
    assert np.array_equal(k, ref["keys"]), f"{label}: keys differ"
    if k.shape[0] == 0:
        return
    span = np.abs(ref["pb"] - ref["pa"])
    slack = 8 * U * (abs(level) + np.abs(ref["fa"]) + np.abs(ref["fb"])) / np.abs(ref["fb"] - ref["fa"])
    bound = span * slack[:, None] + 4 * U * np.maximum(np.abs(ref["pa"]), np.abs(ref["pb"]))
    err = np.abs(v.astype(np.float64) - ref["vertices"])
    assert (err <= bound).all(), f"{label}: a vertex is {float((err / np.maximum(bound, 1e-300)).max()):.2f} times its bound away"


def _counts_gpu(vol, level):
    """The count pass on its own, through the C-ABI."""
    from gspl_amd import _lib as L
    dev = _dev()
    X, Y, Z = vol.shape
    t = torch.from_numpy(vol).to(dev)
    counts = torch.full(((X - 1) * (Y - 1) * (Z - 1),), 255, dtype=torch.uint8, device=dev)
    L.call("gspl_mtet_count", X, Y, Z, L.ptr(t), float(level), L.ptr(counts), L.stream())
    return counts.cpu().numpy().astype(np.int64)


def test_marching_tetrahedra_all_256_sign_patterns():
    rng = np.random.default_rng(3)
    origin, step, level = np.array([0.3, -1.2, 2.0], np.float32), np.array([0.5, 0.25, 1.5], np.float32), 0.125
    total = 0
    for pattern in range(256):
        inside = np.array([(pattern >> m) & 1 for m in range(8)], bool).reshape(2, 2, 2)
        mag = rng.uniform(0.05, 1.0, (2, 2, 2))
        vol = (level + np.where(inside, -mag, mag)).astype(np.float32)
        ref, v, k = _mtet_both(vol, level, origin, step)
        _check_soup(ref, v, k, level, f"pattern {pattern}")
        total += k.shape[0] // 3
        assert (pattern in (0, 255)) == (k.shape[0] == 0)
    assert total > 256 * 4


@pytest.mark.parametrize("name", ["random 3x2x5", "sphere 9", "sphere 17", "torus 24", "X = 1"])
def test_marching_tetrahedra_against_the_oracle(name):
    level = 0.0
    if name == "random 3x2x5":
        vol = np.random.default_rng(11).normal(size=(3, 2, 5)).astype(np.float32)
        origin, step, level = np.array([1.0, -2.0, 0.5], np.float32), np.array([0.1, 0.3, 0.2], np.float32), 0.2
    elif name == "X = 1":
        vol = np.random.default_rng(12).normal(size=(1, 4, 4)).astype(np.float32)
        origin, step = np.zeros(3, np.float32), np.ones(3, np.float32)
    elif name == "torus 24":
        vol, origin, step = MO.torus_volume(24)
    else:
        vol, origin, step = MO.sphere_volume(int(name.split()[1]))
    ref, v, k = _mtet_both(vol, level, origin, step)
    if name == "X = 1":
        assert k.shape[0] == 0 and v.shape == (0, 3)
        return
    assert np.array_equal(_counts_gpu(vol, level), ref["counts"]), f"{name}: triangles per cell differ"
    assert ref["counts"].max() <= 12 and ref["counts"].sum() > 0
    _check_soup(ref, v, k, level, name)


@pytest.mark.parametrize("name, chi, analytic", [("sphere 9", 2, None), ("sphere 17", 2, 4 / 3 * math.pi * 0.5 ** 3),
                                                 ("torus 24", 0, 2 * math.pi ** 2 * 0.5 * 0.2 ** 2)])
def test_indexed_mesh_topology(name, chi, analytic):
    from gspl_amd import ops
    dev = _dev()
    vol, origin, step = MO.torus_volume(24) if name == "torus 24" else MO.sphere_volume(int(name.split()[1]))
    v, f, keys = ops.marching_tetrahedra(torch.from_numpy(vol).to(dev), 0.0, origin.tolist(), step.tolist())
    assert f.dtype == torch.int64 and v.shape[0] == keys.shape[0] and bool((keys[1:] > keys[:-1]).all())
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert MO.is_closed_oriented(f), f"{name}: not a closed oriented 2-manifold"
    assert MO.euler(v.shape[0], f) == chi
    volume = MO.signed_volume(v, f)
    assert volume > 0
    if analytic is not None:
        assert abs(volume / analytic - 1) <= 0.03, f"{name}: volume {volume:.5f}, analytic {analytic:.5f}"


def test_two_blocks_merge_to_the_bits_of_one():
    from gspl_amd import ops
    dev = _dev()
    vol, origin, step = MO.sphere_volume(17)
    t = torch.from_numpy(vol).to(dev)
    o, s = origin.tolist(), step.tolist()
    whole = ops.marching_tetrahedra(t, 0.0, o, s)
    a = ops.marching_tetrahedra_soup(t[:9].contiguous(), 0.0, o, s, global_dims=(17, 17, 17), block_offset=(0, 0, 0))
    b = ops.marching_tetrahedra_soup(t[8:].contiguous(), 0.0, o, s, global_dims=(17, 17, 17), block_offset=(8, 0, 0))
    assert a[1].numel() > 0 and b[1].numel() > 0
    merged = ops.index_soup(torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]]))
    assert torch.equal(merged[2], whole[2]) and torch.equal(merged[0], whole[0])                 # the vertex set, bit for bit
    order = lambda f: f[np.lexsort(f.T[::-1])]
    assert np.array_equal(order(merged[1].cpu().numpy()), order(whole[1].cpu().numpy()))         # the face set
    # a block on its own agrees with the oracle run as that block
    ref = MO.marching_tetrahedra(vol[8:], 0.0, origin, step, (17, 17, 17), (8, 0, 0))
    _check_soup(ref, b[0].cpu().numpy(), b[1].cpu().numpy(), 0.0, "block 8..16")


# ---- the public pipeline --------------------------------------------------------------------------------------------------------------------
def _three_part_mesh(dev):
    """Two disjoint spheres (17^3 and 9^3 lattices) and a 24-face floater (a one-node blob), as one indexed mesh."""
    from gspl_amd import ops
    parts = []
    for n, shift in ((17, 0.0), (9, 5.0)):
        vol, origin, step = MO.sphere_volume(n)
        v, f, _ = ops.marching_tetrahedra(torch.from_numpy(vol).to(dev), 0.0, (origin + shift).tolist(), step.tolist())
        parts.append((v, f))
    blob = np.ones((3, 3, 3), np.float32)
    blob[1, 1, 1] = -1.0
    v, f, _ = ops.marching_tetrahedra(torch.from_numpy(blob).to(dev), 0.0, (20.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert f.shape[0] == 24
    parts.append((v, f))
    offsets = np.cumsum([0] + [p[0].shape[0] for p in parts])
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] + int(o) for p, o in zip(parts, offsets)]), [p[1].shape[0] for p in parts]


def test_keep_largest_clusters():
    from gspl_amd import mesh
    dev = _dev()
    v, f, sizes = _three_part_mesh(dev)
    assert sizes[0] > sizes[1] > 50 > sizes[2] == 24
    v1, f1 = mesh.keep_largest_clusters(v, f, cluster_to_keep=1)
    assert f1.shape[0] == sizes[0] and float(v1[:, 0].max()) < 2.0 and int(f1.max()) == v1.shape[0] - 1
    assert MO.is_closed_oriented(f1.cpu().numpy())
    v2, f2, c2 = mesh.keep_largest_clusters(v, f, colors=v.clone())                              # defaults: fewer than 50 clusters, no raise
    assert f2.shape[0] == sizes[0] + sizes[1] and float(v2[:, 0].max()) < 10.0 and torch.equal(c2, v2)
    v3, f3 = mesh.keep_largest_clusters(v, f, cluster_to_keep=7, min_triangles=1)
    assert f3.shape[0] == sum(sizes) and v3.shape[0] == v.shape[0]


def _cameras(full, w2c, dev):
    return [types.SimpleNamespace(full_projection=torch.from_numpy(full[i]).to(dev), world_to_camera=torch.from_numpy(w2c[i]).to(dev))
            for i in range(full.shape[0])]


def _radii_of_largest(v, f, centre=(0.0, 0.0, 0.0)):
    labels, sizes = MO.components(f)
    r = np.linalg.norm(np.asarray(v, np.float64) - np.asarray(centre), axis=-1)
    return r[np.unique(np.asarray(f)[labels == 0])], sizes


def _all_components_closed(f):
    labels, sizes = MO.components(f)
    return all(MO.is_closed_oriented(f[labels == c]) for c in range(sizes.shape[0]))


@functools.lru_cache(maxsize=None)
def _e2e_scene():
    full, w2c, geo = MO.orbit_cameras(24, 64, 64)
    depth, rgb = MO.sphere_maps(geo, 64, 64, perturb=0.0)
    return full, w2c, depth, rgb


def test_extract_mesh_bounded_end_to_end():
    from gspl_amd import mesh
    dev = _dev()
    full, w2c, depth, rgb = _e2e_scene()
    voxel = 0.05
    args = dict(voxel_size=voxel, sdf_trunc=5 * voxel, depth_trunc=4.0)
    ov, of = MO.extract(full, depth, (-0.8,) * 3, (0.8,) * 3, (33, 33, 33), **args)
    oradii, osizes = _radii_of_largest(ov, of)
    assert osizes.shape[0] >= 2 and _all_components_closed(of)           # the shell behind the truncation band is expected
    assert 0.5 - 1.5 * voxel < oradii.min() < oradii.max() < 0.5 + 1.5 * voxel
    maps = mesh.stack_maps(list(torch.from_numpy(rgb).to(dev)), list(torch.from_numpy(depth).to(dev)))
    v, f, c = mesh.extract_mesh_bounded(maps, _cameras(full, w2c, dev), center=(0.0, 0.0, 0.0), radius=0.8, **args)
    assert c.shape == v.shape and f.dtype == torch.int64
    fn = f.cpu().numpy()
    assert _all_components_closed(fn)
    kv, kf = mesh.keep_largest_clusters(v, f, 1)
    assert MO.euler(kv.shape[0], kf.cpu().numpy()) == 2 and MO.signed_volume(kv.cpu().numpy(), kf.cpu().numpy()) > 0
    radii = np.linalg.norm(kv.cpu().numpy().astype(np.float64), axis=-1)
    print(f"bounded: oracle components {osizes.tolist()}, radii [{oradii.min():.4f}, {oradii.max():.4f}]; GPU {fn.shape[0]} faces, kept "
          f"{kf.shape[0]}, radii [{radii.min():.4f}, {radii.max():.4f}]")
    assert oradii.min() - 0.05 * voxel <= radii.min() and radii.max() <= oradii.max() + 0.05 * voxel


def test_extract_mesh_unbounded_end_to_end():
    from gspl_amd import mesh
    dev = _dev()
    full, w2c, depth, rgb = _e2e_scene()
    rng = np.random.default_rng(4)
    d = rng.normal(size=(2000, 3))
    means = (d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(0.5, 0.75, (2000, 1))).astype(np.float32)
    model = types.SimpleNamespace(get_xyz=torch.from_numpy(means).to(dev))
    resolution, crop = 32, 16
    voxel = RADIUS * 2 / resolution
    centre = np.asarray(CENTER, np.float32)
    R = min(float(np.quantile(np.linalg.norm(MO.contract_np((means.astype(np.float64) - centre) / RADIUS), axis=-1), 0.95)) + 0.01, 1.9)
    n = (resolution // crop) * (crop - 1) + 1
    ov, of = MO.extract(full, depth, (-R,) * 3, (R,) * 3, (n, n, n), center=CENTER, radius=RADIUS, voxel_size=voxel, contract=True)
    ov = MO.uncontract_np(ov) * RADIUS + centre.astype(np.float64)
    oradii, osizes = _radii_of_largest(ov, of)
    assert _all_components_closed(of)
    maps = mesh.stack_maps(list(torch.from_numpy(rgb).to(dev)), list(torch.from_numpy(depth).to(dev)))
    cams = _cameras(full, w2c, dev)
    v, f, c = mesh.extract_mesh_unbounded(maps, (torch.tensor(CENTER), RADIUS), cams, model, resolution=resolution, crop=crop)
    fn = f.cpu().numpy()
    assert _all_components_closed(fn)                                     # eight blocks merged without a seam
    kv, kf, kc = mesh.keep_largest_clusters(v, f, 1, colors=c)
    assert MO.euler(kv.shape[0], kf.cpu().numpy()) == 2
    radii = np.linalg.norm(kv.cpu().numpy().astype(np.float64), axis=-1)
    print(f"unbounded: oracle components {osizes.tolist()}, radii [{oradii.min():.4f}, {oradii.max():.4f}]; GPU {fn.shape[0]} faces, kept "
          f"{kf.shape[0]}, radii [{radii.min():.4f}, {radii.max():.4f}]")
    assert oradii.min() - 0.05 * voxel <= radii.min() and radii.max() <= oradii.max() + 0.05 * voxel
    # the colouring fusion: the oracle at the GPU's own vertices
    ref = MO.fuse(v.cpu().numpy(), full, depth, rgb, voxel_size=voxel)
    firm = ~ref["flagged"]
    # (vacuity guard, not the 2 % cap of the fusion cases: these samples all lie ON the surface and are seen by 24 views, every one of
    # which has them on its silhouette somewhere, where the taps' spread makes the truncation test fragile; nine in ten must be compared)
    assert ref["flagged"].mean() <= 0.10 and float((ref["weight"] > 1).mean()) > 0.3
    cerr = np.abs(c.cpu().numpy().astype(np.float64) - ref["color"]).max(-1)
    assert (cerr[firm] <= KAPPA * U * (ref["s_rgb"][firm] + 4)).all()
    assert float(kc.max()) > 0.5

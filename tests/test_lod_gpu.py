"""`ops.lod_select` / `ops.lod_gather` (include/gspl_hip.h section 26, csrc/lod.hip, ops/lod.py), `gspl_amd.lod` and the
`HipPartitionLoDRenderer` plugin against the fp64 oracle tests/lod_oracle.py, which tests/test_lod.py pins to the reference's own run
(distances, levels) and to a linear programme (visibility).  Nothing here reads the reference tree.

Tolerances.  eps32 = 2^-23 (one ulp of 1.0; a rounded operation errs by at most half of it, so every count below has a factor 2 of room
for second-order terms).  The inputs are float32 values, which the oracle widens exactly.

  distance    p_j = (c @ T)_j is a 3-term dot product: 3 products and 2 sums, 5 roundings relative to M_j = sum_i |c_i T_ij|.
              d_j = max(max(min_j - p_j, p_j - max_j), 0): the subtraction adds 1 rounding relative to |d_j|; max is exact and the clamp a
              contraction.  sqrt(d_x^2 + d_y^2): the squares and the sum are 2 roundings relative to d^2, halved by the root (1), + the
              root (1): 2.5 relative to d (DISTANCE_ROUNDINGS), and |dd / dd_j| <= 1.  Together
                  |distance - ref| <= eps32 [sum_j (5 M_j + |d_j|) + 2.5 d].
  lod         exact: the test asserts BEFORE the GPU runs that every oracle distance is at least 1e-4 partition sizes from every
              threshold, and that this margin exceeds the distance bound.  dst_start and the total are then exact too (integers).
  visible     a point in camera space is 3 products and 3 sums (6 roundings relative to its majorant sum_i |b_i M_ij| + |t_j|; a frustum
              corner, (u - cx) / fx * depth with depth = 10 max(distance), has 4 and the distance's own): 6 eps32 M with M the largest
              l1 majorant of the 16 points.  Its shadow on a unit axis adds the dot product's 5: 11 eps32 M, and a gap is the difference
              of two shadows: 22 eps32 M.  The axis itself: an edge is a difference of two points (12 + 1), a cross product of two of
              them two products and a difference each (2 x 13 + 3), the normalisation 3.5: at most 33 roundings relative to |a| |b|,
              which for an axis whose |a x b| is not small against |a| |b| turns a shadow of extent <= 2 M by 66 eps32 M.  Together
              88, rounded up: |gap - ref| <= 128 eps32 M (GAP_ROUNDINGS).  `visible` must equal the oracle's wherever the oracle's largest
              gap is further than that from zero; the partitions it excludes are counted, printed, and at most 1 % of a case's.
  gather      bit-equal to torch.cat of the chosen slices, rows beyond n untouched, two runs the same bits.
The GPU tests never widen these."""
import numpy as np
import pytest
import torch

import lod_oracle as LO
from fakes import FakeCamera
from oracle import gsplat_oracle as O
from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -23
DISTANCE_ROUNDINGS, GAP_ROUNDINGS = 2.5, 128
EXCLUDED_CAP = 0.01
SIZE = 8.0                                             # the partitions' side length
MARGIN = 1e-4 * SIZE
BLOCK = 256                                            # threads of the selecting workgroup (csrc/lod.hip)
PARTITIONS = [1, 2, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 1000]
WIDTH, HEIGHT, FX, FY, CX, CY = 64, 48, 50.0, 52.0, 31.0, 25.0
PROPERTIES = ("means", "shs", "opacities", "scales", "rotations")


def rotation(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def scene(P, L, seed=3):
    """P partitions of side 8 on a square grid in the oriented frame (a rotated world), boxes between two random heights, L levels with
    random segment lengths 0 .. 40 and thresholds at 0.6, 1.7, 3.3 partition sizes (the first L - 1 of them).  float32 values."""
    rng = np.random.default_rng(seed + 17 * P + L)
    cols = int(np.ceil(np.sqrt(P)))
    ij = np.stack([np.arange(P) % cols, np.arange(P) // cols], -1).astype(np.float64)
    box_min = (ij * SIZE - 0.5 * cols * SIZE).astype(np.float32)
    box_max = (box_min + np.float32(SIZE)).astype(np.float32)
    T = rotation([0.9, 0.1, -0.2, 0.3]).astype(np.float32)          # world -> oriented frame: p = c @ T
    z_lo = rng.uniform(-2.0, -0.5, P)
    z_hi = rng.uniform(0.5, 3.0, P)
    ring = np.stack([box_min, np.stack([box_min[:, 0], box_max[:, 1]], -1), box_max, np.stack([box_max[:, 0], box_min[:, 1]], -1)], 1)   # [P, 4, 2]
    top = np.concatenate([ring, np.broadcast_to(z_hi[:, None, None], (P, 4, 1))], -1)
    bottom = np.concatenate([ring, np.broadcast_to(z_lo[:, None, None], (P, 4, 1))], -1)
    corners = (np.concatenate([top, bottom], 1) @ T.astype(np.float64).T).astype(np.float32)           # world space
    thresholds = (np.array([0.6, 1.7, 3.3])[:L - 1] * SIZE).astype(np.float32)
    lengths = rng.integers(0, 41, L * P)
    seg_start = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return dict(P=P, L=L, box_min=box_min, box_max=box_max, transform=T, corners=corners, thresholds=thresholds, seg_start=seg_start)


def camera(position, target, up=(0.0, 0.0, 1.0)):
    """-> (camera_center [3], world_to_camera [4, 4] in the reference's transposed storage), float32; +z looks at `target`."""
    c, t = np.asarray(position, np.float64), np.asarray(target, np.float64)
    z = (t - c) / np.linalg.norm(t - c)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], 0)                         # x_cam = R (x_world - c)
    M = np.eye(4)
    M[:3, :3], M[3, :3] = R.T, -R @ c
    M = M.astype(np.float32)
    centre = (-M[3, :3].astype(np.float64) @ np.linalg.inv(M[:3, :3].astype(np.float64))).astype(np.float32)
    return centre, M


def cameras(s):
    """Three views in world space: from above the grid looking across it, from outside looking in, and from outside looking AWAY (every
    partition behind the camera)."""
    back = np.linalg.inv(s["transform"].astype(np.float64))        # oriented frame -> world
    half = 0.5 * SIZE * np.ceil(np.sqrt(s["P"]))
    at = lambda *p: np.array(p) @ back
    return {"across": camera(at(0.37 * half + 0.123, -0.21 * half + 0.071, 6.3), at(0.9 * half, 0.8 * half, 0.0)),
            "inwards": camera(at(-half - 11.17, -half - 5.43, 9.1), at(0.0, 0.0, 0.0)),
            "away": camera(at(-half - 11.17, -half - 5.43, 9.1), at(-3 * half - 40.0, -2 * half - 30.0, 12.0))}


def expected(s, centre, w2c, filter_on):
    """The oracle's frame, with the bounds of the header."""
    c64, T64 = centre.astype(np.float64), s["transform"].astype(np.float64)
    d = LO.distances(centre, s["transform"], s["box_min"], s["box_max"])
    p = (c64 @ T64)[:2]
    major = (np.abs(c64)[:, None] * np.abs(T64))[:, :2].sum(0)
    dj = np.maximum(np.maximum(s["box_min"] - p, p - s["box_max"]), 0.0)
    d_bound = EPS * ((5 * major[None] + dj).sum(-1) + DISTANCE_ROUNDINGS * d)
    lod = LO.levels(d, s["thresholds"].astype(np.float64), s["L"])
    out = dict(distance=d, distance_bound=d_bound, lod=lod, margin=LO.threshold_margin(d, s["thresholds"]))
    if filter_on:
        visible, sep = LO.visibility(d, s["corners"], w2c, FX, FY, CX, CY, WIDTH, HEIGHT)
        M64 = w2c.astype(np.float64)
        F = LO.frustum(FX, FY, CX, CY, WIDTH, HEIGHT, LO.FAR_FACTOR * d.max())
        box_major = np.abs(s["corners"].astype(np.float64)) @ np.abs(M64[:3, :3]) + np.abs(M64[3, :3])
        out.update(visible=visible, separation=sep, gap_bound=GAP_ROUNDINGS * EPS * max(np.abs(F).sum(-1).max(), box_major.sum(-1).max()))
    else:
        out.update(visible=np.ones(s["P"], bool))
    out["dst_start"] = LO.dst_start(lod, out["visible"], s["seg_start"], s["P"])
    return out


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def run_select(s, centre, w2c, filter_on, prev=None, thresholds=None):
    from gspl_amd import ops
    P = s["P"]
    prev_lod, prev_visible = prev if prev is not None else (torch.full((P,), 127, dtype=torch.int8, device=DEV), torch.ones(P, dtype=torch.uint8, device=DEV))
    K = torch.tensor([[FX, 0.0, CX], [0.0, FY, CY], [0.0, 0.0, 1.0]], device=DEV)
    return ops.lod_select(dev(s["seg_start"]), dev(centre), dev(s["transform"]), dev(s["box_min"]), dev(s["box_max"]),
                          dev(s["thresholds"] if thresholds is None else thresholds), prev_lod, prev_visible, dev(s["corners"]), dev(w2c), K,
                          WIDTH, HEIGHT, filter_on)


@pytest.mark.parametrize("filter_on", [False, True], ids=["all", "frustum"])
@pytest.mark.parametrize("L", [1, 2, 4])
@pytest.mark.parametrize("P", PARTITIONS)
def test_select_against_the_oracle(P, L, filter_on):
    s = scene(P, L)
    for name, (centre, w2c) in cameras(s).items():
        want = expected(s, centre, w2c, filter_on)
        assert want["margin"].min() >= MARGIN and (want["margin"] > want["distance_bound"]).all(), (name, want["margin"].min())      # before the GPU runs
        distance, lod, visible, dst_start, record = run_select(s, centre, w2c, filter_on)
        distance, lod, visible = distance.cpu().numpy(), lod.cpu().numpy(), visible.cpu().numpy().astype(bool)
        excess = np.abs(distance - want["distance"]) - want["distance_bound"]
        print(f"P {P} L {L} {name}: distance error / bound {np.max(np.abs(distance - want['distance']) / want['distance_bound']):.3f}")
        assert excess.max() <= 0, (name, int(excess.argmax()))
        assert np.array_equal(lod, want["lod"]), name
        sure = np.ones(P, bool)
        if filter_on:
            sure = np.abs(want["separation"]) > want["gap_bound"]
            sure[int(np.argmin(want["distance"]))] = True
            print(f"P {P} L {L} {name}: {int(want['visible'].sum())} visible, {int((~sure).sum())} within {want['gap_bound']:.2e} of touching")
            assert (~sure).sum() <= EXCLUDED_CAP * P, name
        assert np.array_equal(visible[sure], want["visible"][sure]), (name, np.nonzero(visible != want["visible"])[0][:8])
        if sure.all():
            assert np.array_equal(dst_start.cpu().numpy(), want["dst_start"]), name
            assert record.tolist() == [int(want["dst_start"][-1]), 1], name
        else:       # the scan of what the kernel itself chose, and its total
            own = LO.dst_start(lod, visible, s["seg_start"], P)
            assert np.array_equal(dst_start.cpu().numpy(), own), name
            assert record.tolist() == [int(own[-1]), 1], name


def test_the_nearest_partition_is_visible_behind_the_camera():
    s = scene(65, 2)
    centre, w2c = cameras(s)["away"]
    want = expected(s, centre, w2c, True)
    nearest = int(np.argmin(want["distance"]))
    assert want["separation"].min() > want["gap_bound"] and want["visible"].sum() == 1          # everything lies behind the camera
    _, _, visible, dst_start, record = run_select(s, centre, w2c, True)
    assert visible.cpu().numpy().nonzero()[0].tolist() == [nearest]
    i = int(want["lod"][nearest]) * 65 + nearest
    assert record.tolist()[0] == int(s["seg_start"][i + 1] - s["seg_start"][i]) == int(dst_start[-1])


def test_changed_follows_the_selection():
    """1 on the first frame (the stored levels are 127), 0 on a repeat, 1 after ONE threshold is moved across ONE partition's distance."""
    s = scene(257, 4)
    centre, w2c = cameras(s)["across"]
    want = expected(s, centre, w2c, False)
    _, lod, visible, _, record = run_select(s, centre, w2c, False)
    assert record.tolist()[1] == 1
    _, lod2, visible2, dst2, record2 = run_select(s, centre, w2c, False, prev=(lod, visible))
    assert record2.tolist() == [int(want["dst_start"][-1]), 0] and torch.equal(lod, lod2) and torch.equal(visible, visible2)
    # the threshold between levels 1 and 2 moves just below the largest distance under it: that one partition becomes level 2
    d = np.sort(want["distance"][want["lod"] == 1])
    assert len(d) >= 2 and d[-1] - d[-2] > MARGIN
    moved = s["thresholds"].copy()
    moved[1] = np.float32(0.5 * (d[-1] + d[-2]))
    _, lod3, _, _, record3 = run_select(s, centre, w2c, False, prev=(lod, visible), thresholds=moved)
    differing = (lod3 != lod).cpu().numpy().nonzero()[0]
    assert record3.tolist()[1] == 1 and differing.tolist() == [int(np.argmax(np.where(want["lod"] == 1, want["distance"], -1.0)))]
    assert int(lod3[differing[0]]) == 2
    # with the filter the flag also follows `visible`
    _, lod4, visible4, _, record4 = run_select(s, centre, w2c, True, prev=(lod, visible))
    assert record4.tolist()[1] == int(not bool(visible4.all()))


# ---- the gather ----------------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 2, 3, 5, 64, 257, 1000)
POISON = 0x7FC0DEAD                                    # an int32 pattern no copy produces (a NaN as float32)


def table_arrays(seg_start, K, seed):
    g = torch.Generator().manual_seed(seed)
    R = int(seg_start[-1])
    return {k: torch.randn((R,) + w, generator=g).to(DEV) for k, w in (("means", (3,)), ("shs", (K, 3)), ("opacities", (1,)), ("scales", (3,)),
                                                                     ("rotations", (4,)))}


@pytest.mark.parametrize("first", [1, 2, 3])
@pytest.mark.parametrize("K", [1, 4, 16])
def test_gather_is_bit_equal_to_concatenation(K, first):
    """L = 3, P = 24; lengths drawn from {0, 1, 2, 3, 5, 64, 257, 1000}; the table's first segment has 1, 2 or 3 rows, so that with 12-
    and 4-byte rows later segments start on every 16-byte phase, in the source and (through the chosen lengths) in the destination;
    a quarter of the partitions invisible; destination buffers 100 rows larger than needed, poisoned."""
    from gspl_amd import ops
    L, P = 3, 24
    rng = np.random.default_rng(100 * K + first)
    lengths = rng.choice(LENGTHS, L * P)
    lengths[0] = first
    lengths[rng.permutation(L * P)[:len(LENGTHS)]] = LENGTHS          # every length at least once
    lengths[0] = first
    seg_start = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    arrays = table_arrays(seg_start, K, seed=K + first)
    phases = set()
    for trial in range(2):
        lod = rng.integers(0, L, P)
        visible = rng.random(P) > 0.25
        if trial == 0:
            lod[0], visible[0] = 0, True              # the short first segment leads the destination too
        dst_start = LO.dst_start(lod, visible, seg_start, P)
        n = int(dst_start[-1])
        chosen = [p for p in range(P) if visible[p] and dst_start[p + 1] > dst_start[p]]
        phases |= {(int(seg_start[lod[p] * P + p]) * 3 % 4, int(dst_start[p]) * 3 % 4) for p in chosen}
        out = [torch.full((n + 100,) + tuple(arrays[k].shape[1:]), 0, dtype=torch.int32, device=DEV).fill_(POISON).view(torch.float32) for k in PROPERTIES]
        got = ops.lod_gather(dev(seg_start), dev(lod, torch.int8), dev(dst_start), n, *[arrays[k] for k in PROPERTIES], out=out)
        again = ops.lod_gather(dev(seg_start), dev(lod, torch.int8), dev(dst_start), n, *[arrays[k] for k in PROPERTIES])
        for k, o, a in zip(PROPERTIES, got, again):
            want = torch.cat([arrays[k][seg_start[lod[p] * P + p]:seg_start[lod[p] * P + p + 1]] for p in range(P) if visible[p]] + [arrays[k][:0]])
            assert want.shape[0] == n and tuple(a.shape) == tuple(want.shape), k
            assert torch.equal(o[:n].view(torch.int32), want.view(torch.int32)), (k, trial)
            assert torch.equal(a.view(torch.int32), want.view(torch.int32)), (k, trial)
            assert bool((o[n:].view(torch.int32) == POISON).all()), (k, trial)
    assert len({s for s, _ in phases}) == 4 and len({d for _, d in phases}) == 4, phases


def test_gather_of_nothing_and_of_one_row():
    from gspl_amd import ops
    seg_start = np.array([0, 1, 1], np.int64)          # L = 1, P = 2: one row, then an empty segment
    arrays = table_arrays(seg_start, 4, seed=5)
    lod = torch.zeros(2, dtype=torch.int8, device=DEV)
    none = ops.lod_gather(dev(seg_start), lod, dev(np.zeros(3, np.int64)), 0, *[arrays[k] for k in PROPERTIES])
    assert [tuple(t.shape) for t in none] == [(0, 3), (0, 4, 3), (0, 1), (0, 3), (0, 4)]
    one = ops.lod_gather(dev(seg_start), lod, dev(np.array([0, 1, 1], np.int64)), 1, *[arrays[k] for k in PROPERTIES])
    assert all(torch.equal(o, arrays[k]) for k, o in zip(PROPERTIES, one))


# ---- the selector and the plugin -----------------------------------------------------------------------------------------------------
W, H, N = 64, 48, 2000


def lod_scene():
    """~2 000 Gaussians of the synthetic scene in 2 x 2 partitions of the x-y plane; level l keeps every 2^l-th Gaussian of a partition."""
    means, scales, quats, opac, shs = O.synthetic_scene(N, seed=41)
    scales = scales * 4
    box_min = torch.tensor([[-1.3, -1.3], [0.0, -1.3], [-1.3, 0.0], [0.0, 0.0]])
    box_max = box_min + 1.3
    cell = (means[:, 0] >= 0).long() + 2 * (means[:, 1] >= 0).long()
    levels = []
    for l in range(3):
        level = []
        for p in range(4):
            rows = (cell == p).nonzero()[:, 0][::2 ** l]
            level.append({"means": means[rows], "shs": shs[rows], "opacities": opac[rows], "scales": scales[rows], "rotations": quats[rows]})
        levels.append(level)
    return levels, box_min, box_max


class CatModel:
    """The same frozen model by torch.cat of the chosen segments."""
    is_pre_activated = True

    def __init__(self, levels, choice):
        self.p = {k: torch.cat([levels[l][p][k] for p, l in enumerate(choice)]).to(DEV) for k in PROPERTIES}
        self.active_sh_degree = 3

    get_xyz = property(lambda s: s.p["means"])
    get_features = property(lambda s: s.p["shs"])

    def get_means(self): return self.p["means"]
    def get_scales(self): return self.p["scales"]
    def get_rotations(self): return self.p["rotations"]
    def get_opacities(self): return self.p["opacities"]


def plugin_camera(x, y):
    """The synthetic camera (looking along +z from z = -4) moved to (x, y) in the plane of the partitions."""
    cam = O.synthetic_camera(W, H, 60.0, 59.0)
    w2c = cam["world_to_camera"].clone()
    w2c[3, 0], w2c[3, 1] = -x, -y
    cam["world_to_camera"] = w2c
    cam["camera_center"] = torch.linalg.inv(w2c)[3, :3]
    return FakeCamera(cam, DEV)


def test_plugin_renders_the_concatenated_model_and_follows_the_camera():
    from gspl_amd.lod import LoDTable
    from gspl_amd.renderers import HipGSplatV1Renderer, HipPartitionLoDRendererModule
    levels, box_min, box_max = lod_scene()
    table = LoDTable(levels, device=DEV)
    thresholds = torch.tensor([0.5, 1.5])
    module = HipPartitionLoDRendererModule.from_table(table, box_min, box_max, thresholds=thresholds)
    bg = torch.tensor([0.1, 0.3, 0.6], device=DEV)
    lengths = lambda choice: sum(table.segment_length(l, p) for p, l in enumerate(choice))

    def choice_at(x, y):
        d = LO.distances(np.array([x, y, -4.0], np.float32), np.eye(3), box_min.numpy(), box_max.numpy())
        assert LO.threshold_margin(d, thresholds.numpy()).min() > 1e-3
        return LO.levels(d, thresholds.numpy(), 3).tolist()

    # above partition 3: it is at distance 0, its neighbours at 0.65, the opposite one at 0.92
    first = choice_at(0.65, 0.65)
    assert first == [1, 1, 1, 0]
    with torch.no_grad():
        out = module(plugin_camera(0.65, 0.65), None, bg)
        n_first, image = out["n_gaussians"], out["render"].clone()      # (a later frame may reuse the buffer)
        ref = HipGSplatV1Renderer().instantiate()(plugin_camera(0.65, 0.65), CatModel(levels, first), bg)
    assert n_first == lengths(first) == module.gaussian_model.n_gaussians and tuple(image.shape) == (3, H, W)
    assert torch.equal(image.view(torch.int32), ref["render"].view(torch.int32)) and float(image.std()) > 0.01
    assert all(k in out and out[k] >= 0 for k in ("time", "render_time_with_lod_preprocess", "render_time"))
    assert (module.selector.n_selects, module.selector.n_gathers) == (1, 1)

    # a second frame from the same pose: selected again, not gathered again
    with torch.no_grad():
        same = module(plugin_camera(0.65, 0.65), None, bg)
    assert (module.selector.n_selects, module.selector.n_gathers) == (2, 1) and same["n_gaussians"] == n_first
    assert torch.equal(same["render"], image)

    # across ONE threshold: towards partition 1 (y < 0), whose distance falls from 0.65 to 0.1, below 0.5; nothing else changes level
    step = choice_at(0.65, 0.1)
    assert [p for p in range(4) if first[p] != step[p]] == [1] and step[1] == 0
    with torch.no_grad():
        moved = module(plugin_camera(0.65, 0.1), None, bg)
    assert moved["n_gaussians"] - n_first == table.segment_length(0, 1) - table.segment_length(1, 1) != 0
    assert module.selector.n_gathers == 2

    # freeze keeps the previous set, whatever the camera does
    module.config.freeze = True
    with torch.no_grad():
        frozen = module(plugin_camera(0.65, 0.65), None, bg)
        frozen_image = frozen["render"].clone()
        ref = HipGSplatV1Renderer().instantiate()(plugin_camera(0.65, 0.65), CatModel(levels, step), bg)
    assert frozen["n_gaussians"] == moved["n_gaussians"] and module.selector.n_gathers == 2 and module.selector.n_selects == 4
    assert torch.equal(frozen_image.view(torch.int32), ref["render"].view(torch.int32))
    module.config.freeze = False
    with torch.no_grad():
        thawed = module(plugin_camera(0.65, 0.65), None, bg)
    assert thawed["n_gaussians"] == n_first and module.selector.n_gathers == 3 and torch.equal(thawed["render"], image)


def test_plugin_with_the_visibility_filter_drops_what_the_oracle_drops():
    from gspl_amd.lod import LoDTable
    from gspl_amd.renderers import HipPartitionLoDRenderer, HipPartitionLoDRendererModule
    levels, box_min, box_max = lod_scene()
    ring = torch.stack([box_min, torch.stack([box_min[:, 0], box_max[:, 1]], -1), box_max, torch.stack([box_max[:, 0], box_min[:, 1]], -1)], 1)
    corners = torch.cat([torch.cat([ring, torch.full((4, 4, 1), z)], -1) for z in (1.3, -1.3)], 1)
    module = HipPartitionLoDRendererModule.from_table(LoDTable(levels, device=DEV), box_min, box_max, thresholds=torch.tensor([0.5, 1.5]), corners=corners,
                                                      config=HipPartitionLoDRenderer(data=None, names=None, visibility_filter=True))
    # far to the side, looking along +z: the frustum (half-width 64 / 120 per unit depth) passes the partitions by
    cam = plugin_camera(9.0, 0.65)
    d = LO.distances(cam.camera_center.cpu().numpy(), np.eye(3), box_min.numpy(), box_max.numpy())
    visible, sep = LO.visibility(d, corners.numpy(), cam.world_to_camera.cpu().numpy(), 60.0, 59.0, W / 2, H / 2, W, H)
    assert np.abs(sep).min() > 1e-3 and 1 <= visible.sum() < 4
    with torch.no_grad():
        out = module(cam, None, torch.zeros(3, device=DEV))
    lod = LO.levels(d, np.array([0.5, 1.5]), 3)
    assert module.is_partition_visible.cpu().numpy().astype(bool).tolist() == visible.tolist()
    assert out["n_gaussians"] == sum(module.table.segment_length(int(l), p) for p, l in enumerate(lod) if visible[p])


class ReferenceLayoutCamera(FakeCamera):
    """The tensors as the reference's `Cameras.__getitem__` hands them out (internal/cameras/cameras.py): `world_to_camera` is a slice of
    `torch.transpose(...)`, a [4, 4] VIEW with strides (1, 4); here `camera_center` is a strided view too (every other element)."""

    def __init__(self, cam, device):
        super().__init__(cam, device)
        self.world_to_camera = self.world_to_camera.T.contiguous().T
        spread = torch.zeros(6, device=device)
        spread[::2] = self.camera_center
        self.camera_center = spread[::2]
        assert self.world_to_camera.stride() == (1, 4) and not self.camera_center.is_contiguous()


def test_plugin_takes_cameras_in_the_reference_layout():
    """Filter on and off, with a rotated camera (so that reading the matrix untransposed would show): the same selection, count and
    image as with contiguous tensors, and the oracle's visibility."""
    from gspl_amd.lod import LoDTable
    from gspl_amd.renderers import HipPartitionLoDRenderer, HipPartitionLoDRendererModule
    levels, box_min, box_max = lod_scene()
    ring = torch.stack([box_min, torch.stack([box_min[:, 0], box_max[:, 1]], -1), box_max, torch.stack([box_max[:, 0], box_min[:, 1]], -1)], 1)
    corners = torch.cat([torch.cat([ring, torch.full((4, 4, 1), z)], -1) for z in (1.3, -1.3)], 1)
    cam = O.synthetic_camera(W, H, 60.0, 59.0)
    angle = 0.45                                     # about the y axis, then 4 back: partitions 0 and 2 (x < 0) leave the frustum
    R = torch.tensor([[np.cos(angle), 0.0, np.sin(angle)], [0.0, 1.0, 0.0], [-np.sin(angle), 0.0, np.cos(angle)]], dtype=torch.float32)
    w2c = torch.eye(4)
    w2c[:3, :3], w2c[3, :3] = R, torch.tensor([-2.6, 0.1, 4.0])
    cam["world_to_camera"], cam["camera_center"] = w2c, torch.linalg.inv(w2c)[3, :3]
    assert not torch.equal(w2c[:3, :3], w2c[:3, :3].T)
    d = LO.distances(cam["camera_center"].numpy(), np.eye(3), box_min.numpy(), box_max.numpy())
    assert LO.threshold_margin(d, np.array([0.5, 1.5])).min() > 1e-3
    lod = LO.levels(d, np.array([0.5, 1.5]), 3)
    visible, sep = LO.visibility(d, corners.numpy(), w2c.numpy(), 60.0, 59.0, W / 2, H / 2, W, H)
    assert np.abs(sep).min() > 1e-3 and 1 <= visible.sum() < 4
    bg = torch.zeros(3, device=DEV)
    for filter_on in (True, False):
        seen = visible if filter_on else np.ones(4, bool)
        images = []
        for camera_class in (FakeCamera, ReferenceLayoutCamera):
            module = HipPartitionLoDRendererModule.from_table(LoDTable(levels, device=DEV), box_min, box_max, thresholds=torch.tensor([0.5, 1.5]),
                                                              corners=corners,
                                                              config=HipPartitionLoDRenderer(data=None, names=None, visibility_filter=filter_on))
            with torch.no_grad():
                out = module(camera_class(cam, DEV), None, bg)
            images.append(out["render"].clone())
            assert module.partition_lods.cpu().tolist() == lod.tolist(), (filter_on, camera_class.__name__)
            assert module.is_partition_visible.cpu().numpy().astype(bool).tolist() == seen.tolist(), (filter_on, camera_class.__name__)
            assert out["n_gaussians"] == sum(module.table.segment_length(int(l), p) for p, l in enumerate(lod) if seen[p])
        assert torch.equal(images[0], images[1]) and float(images[0].std()) > 0

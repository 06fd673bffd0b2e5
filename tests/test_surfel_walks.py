"""The HIP surfel (2DGS) rasterizer against the fp64 oracle on the paths the one parity scene of test_surfel_gpu.py never reaches.

  1. "reset": 900 surfels right after an opacity reset (every opacity 0.01), large enough that G >= ~0.7 over the frame: tile lists of
     ~800-870 entries (four staging batches of `surfel_fwd_kernel`, ~27 batches of the backward), no pixel saturating, every pixel
     walking its list to the end and the backward compounding Ti = Tc / (1 - alpha) over 600+ contributors.
  2. "mixed": the reset scene whose surfels behind depth 5.2 are small opaque discs (sigma 2.5 ... 4 px, opacity 0.2 ... 0.8) over the far
     half of the frame's longer side.  Those pixels meet the transmittance stop within a few opaque entries, 100-190 entries before
     their tile's list ends; the near half walks its list to the end.  `last` differs by more than 64 entries within a tile, so the
     backward's `idx < last` skip and its `walk_end` (the block maximum) both decide.  (Opaque surfels that cover the whole frame, or
     forty of sigma 6 ... 16 px in the middle of the column, stop EVERY pixel of these small frames, and a stop reached in steps of
     alpha ~0.008 lands within the oracle's stop margin in ~3 % of the pixels: the opaque ones are small, confined, and last.)
  3. "clamp": the parity scene of test_surfel_gpu.py with sixteen surfels of opacity 0.992 ... 1.0 in front: raw alpha above 0.99 and the
     straight-through backward of the clamp.  (o exp(-rho / 2) > 0.99 needs rho < 2 ln(o / 0.99) <= 0.0201: a disc of 0.09 ... 0.14
     sigma.  200 such pixels from a handful of surfels need sigma of 18 ... 30 px: the surfels are frame-sized, their clamped cores a
     few pixels.)
  4. rotated views: poses with yaw, pitch and roll, every entry of the rotation non-zero, among them a close-up and a view from behind.
     The oracle itself is first shown invariant under the rigid motion that takes such a pose to the identity pose (CPU), then the two
     HIP renders of that pair are compared with each other, then the HIP rasterizer with the oracle, then the renderer plugin with
     the op.

Every scene asserts, from the oracle alone, that it reaches the path it is meant for (`surfel_oracle.render`'s pair statistics).  Bounds
are those of test_surfel_gpu.test_surfel_against_fp64_oracle.  Every test prints its scene statistics, its worst forward error per
channel and its worst / median gradient ratio per input.

MEASURED (scene statistics: the oracle on the CPU; errors: HIP on an MI355X against the oracle, worst over the unflagged pixels /
the rows that are not excused)

  scene          lists     final T             contributors  stopped      pairs 3D / low-pass / clamped  flagged      excused  spread of last
  reset-40x24    799-871   3.4e-4 .. 7.5e-4    799-805       0            767028 / 315 / 0               5 of 960     3        -
  reset-17x33    802-873   3.2e-4 .. 5.4e-4    802-809       0            449917 / 292 / 0               2 of 561     2        -
  mixed-40x24    694-877   1.0e-4 .. 3.1e-3    637-680       513 of 960   624857 / 285 / 0               7 of 960     6        148
  mixed-17x33    694-861   1.0e-4 .. 2.5e-3    638-697       314 of 561   365912 / 296 / 0               2 of 561     2        109
  clamp          24-216    1.0e-4 .. 7.0e-2    4-36          3853 of 6912 125442 / 445 / 269             13 of 6912   12       -
  pose-oblique   2-211     3.2e-4 .. 1         0-29          0            37360 / 3848 / 0               14 of 6912   12       (607 visible)
  pose-close     34-132    6.7e-3 .. 0.98      2-22          0            72230 / 1415 / 0               11 of 6912   10       (501 visible)
  pose-behind    0-202     2.0e-3 .. 1         0-28          0            22295 / 4296 / 0               15 of 6912   12       (614 visible)
  (deterministic mode: 4954 and 4937 per-entry rows in the reset frames)

  forward, worst channel against its bound          colour (2e-5)  alpha (2e-5)  normal (2e-5)  depth (1e-5 x)   median (1e-5 x)  distortion (1e-5 x)
  reset-40x24 / 17x33                               1.4e-6 / 8.9e-7  3.1e-8      2.0e-6         6.5e-6 of 2.6e-5 1.3e-7           5.4e-7 of 1.0e-5
  mixed-40x24 / 17x33                               1.2e-6 / 8.6e-7  3.1e-8      1.6e-6         5.2e-6 of 2.6e-5 1.4e-7           6.0e-7 of 1.0e-5
  clamp (shs / colors_precomp)                      6.1e-7 / 9.0e-7  1.3e-7      3.5e-7         3.2e-6 of 2.1e-5 1.5e-7           6.1e-7 of 1.0e-5
  pose-oblique                                      6.0e-6           5.7e-6      1.5e-5         9.1e-6 of 5.0e-5 2.4e-6           1.9e-7
  pose-close                                        4.6e-6           7.2e-6      9.2e-6         1.6e-5 of 2.8e-5 2.2e-6           1.3e-7
  pose-behind                                       6.8e-6           9.5e-6      1.8e-5         4.9e-5 of 6.4e-5 5.6e-6           1.4e-7

  gradients, worst |got - ref| / (|ref| + rms) (bound 2e-3 per element, median 1e-4; medians measured 0 ... 1.1e-6)
                 means    scales   quats    opacities  shs / colors_precomp  means2d   rows beyond 2e-3
  reset-40x24    9.0e-6   3.0e-5   1.2e-5   2.7e-5     1.1e-6                9.5e-6    0
  reset-17x33    1.4e-5   3.8e-5   1.7e-5   1.6e-5     2.1e-6                1.6e-5    0     (deterministic: the same to two digits)
  mixed-40x24    1.3e-5   6.1e-5   5.9e-6   2.1e-5     1.4e-6                1.9e-5    0     (deterministic: the same to two digits)
  mixed-17x33    5.9e-6   8.9e-5   3.9e-6   1.2e-5     1.3e-6                3.0e-5    0     (deterministic: the same to two digits)
  clamp-shs      1.1e-5   1.4e-5   8.1e-6   9.1e-6     5.6e-6                1.3e-5    0     (10 pixels clamped first: alpha >= 0.991392)
  clamp-precomp  1.2e-5   1.6e-5   8.3e-6   1.9e-5     5.1e-6                1.4e-5    0
  pose-oblique   1.6e-4   3.4e-5   2.7e-4   1.6e-5     1.6e-5                2.0e-4    0
  pose-close     7.4e-5   2.3e-5   8.3e-5   2.4e-5     1.4e-5                7.7e-5    0
  pose-behind    1.4e-3   2.2e-5   1.2e-3   1.2e-5     2.3e-5                3.0e-3    1 (means2d; one row is allowed)

  Under a rotated pose every product of Tu / Tv / Tw = (t_u, t_v, p) . (P N) has three non-zero terms where the identity pose has
  one, and the per-pixel k = x Tw - Tu of a sub-pixel surfel cancels against that rounding: the forward errors are 5-10 x those of
  the identity pose, still inside the bounds.
  The rigid-motion pair on the oracle: 8.5e-14 worst (normal) with an fp64 pose, 3.2e-6 worst (normal y; depth 2.7e-6) with the
  fp32-rounded pose.  The same pair on the HIP rasterizer: colour 1.1e-5, normal 2.3e-5 (bound 4e-5), depth 2.2e-5 (bound 1.0e-4).
  The plugin: `rend_normal` / `surf_depth` bit-equal to the op's maps rotated in torch; with fused_maps 6.0e-8 / 0.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import gsplat_oracle as O
import surfel_oracle as SO
from hip_helpers import reset_opacities
from test_surfel_gpu import H, TOL, W, _grad_check, _oracle, _run_hip, _settings, _special_scene

gpu = pytest.mark.gpu
BG = torch.tensor([0.3, 0.1, 0.6])
ALLMAP_WEIGHTS = torch.tensor([0.02, 0.1, 0.1, 0.1, 0.1, 0.02, 5.0])
CHANNELS = ("depth", "alpha", "normal x", "normal y", "normal z", "median", "distortion")


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def _column_scene(W, H, seed, mixed, n=900):
    """The deep column right after an opacity reset; `mixed`: plus a medium band and an opaque back half."""
    g = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g)
    cam = O.synthetic_camera(W, H, 80.0, 80.0 * 0.97)
    tan = torch.tensor([cam["tanfovx"], cam["tanfovy"]])
    depth = rand(n) * 4 + 2
    xy = (rand(n, 2) * 2 - 1) * tan * depth[:, None] * 0.5
    means = torch.cat([xy, depth[:, None] - 4], dim=1)
    scales = (rand(n, 2) * 0.1 + 0.6) * depth[:, None]
    u = rand(n)
    tiny = u < 0.12                                                 # sub-pixel: 0.05 ... 0.35 px
    scales = torch.where(tiny[:, None], (rand(n, 2) * 0.3 + 0.05) * depth[:, None] / 80, scales)
    axis = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    ang = rand(n) * 0.4                                             # (a 3-sigma disc tilted further crosses the camera plane)
    quats = torch.cat([torch.cos(ang / 2)[:, None], axis * torch.sin(ang / 2)[:, None]], dim=1) * 1.7
    opac = reset_opacities(rand(n, 1) * 0.6 + 0.2)
    shs = torch.randn(n, 16, 3, generator=g) * 0.2
    if mixed:
        # the opaque back: every surfel behind depth 5.2 that is not sub-pixel becomes a small opaque disc (sigma 2.5 ... 4 px) over the far
        # half of the frame's longer side.  There T is ~2e-3 when the walk arrives and falls below the stop within a few of them, in
        # steps of alpha 0.1 ... 0.8; the near half never sees them and walks its list to the end.
        back = (depth > 5.2) & ~tiny
        long_axis = 0 if W >= H else 1
        pos = rand(n, 2) * 2 - 1
        pos[:, long_axis] = rand(n) * 0.95 + 0.05
        xy_back = pos * tan * depth[:, None]
        means = torch.where(back[:, None], torch.cat([xy_back, depth[:, None] - 4], dim=1), means)
        scales = torch.where(back[:, None], (rand(n, 2) * 1.5 + 2.5) * depth[:, None] / 80, scales)
        opac = torch.where(back[:, None], rand(n, 1) * 0.6 + 0.2, opac)
    return (means, scales, quats, opac, shs), cam


def _clamp_scene(seed=41):
    """`_special_scene` plus eighteen surfels of opacity 0.992 ... 1.0 (skewed towards 1) in front of its cloud: sixteen on a jittered
    4 x 4 grid, sigma ~22 px, at view depths 2.0 ... 2.4 in raster order (the cloud starts at 2.7), and two of sigma 10 px at depths
    0.22 and 0.235, in front of the scene's near-plane surfels too, so that some pixels meet a clamped alpha first.  The grid keeps
    the clamped cores (0.14 sigma at most) apart: two clamped alphas in a row leave T = (1 - 0.99)^2, which IS the stop's threshold."""
    (means, scales, quats, opac, shs), cam = _special_scene(seed=seed)
    g = torch.Generator().manual_seed(seed + 1000)
    rand = lambda *s: torch.rand(*s, generator=g)
    k = 16
    depth = torch.cat([2.0 + 0.4 * torch.arange(k) / k, torch.tensor([0.22, 0.235])])
    px = torch.cat([((torch.arange(k) % 4) + 0.5) / 4 * W + (rand(k) - 0.5) * 6, torch.tensor([14.3, 81.6])])
    py = torch.cat([((torch.arange(k) // 4) + 0.5) / 4 * H + (rand(k) - 0.5) * 6, torch.tensor([11.7, 60.4])])
    m = torch.stack([(px - (W - 1) / 2) / 80.0 * depth, (py - (H - 1) / 2) / 78.0 * depth, depth - 4], dim=1)
    sigma = torch.cat([(rand(k, 2) * 0.2 + 0.9) * 22, (rand(2, 2) * 0.2 + 0.9) * 10])
    s = sigma / 0.9 * depth[:, None] / 80                           # (the tests render at scale modifier 0.9)
    axis = torch.nn.functional.normalize(torch.randn(k + 2, 3, generator=g), dim=-1)
    ang = torch.cat([rand(k) * 0.3, torch.tensor([0.02, 0.03])])    # (the two near ones stay clear of the near plane)
    q = torch.cat([torch.cos(ang / 2)[:, None], axis * torch.sin(ang / 2)[:, None]], dim=1)
    o = 1 - 0.008 * rand(k + 2, 1) ** 2
    c = torch.randn(k + 2, shs.shape[1], 3, generator=g) * 0.2
    return (torch.cat([means, m]), torch.cat([scales, s]), torch.cat([quats, q]), torch.cat([opac, o]), torch.cat([shs, c])), cam


def posed_camera(width, height, fx, fy, yaw, pitch, roll, distance, dtype=torch.float32):
    """A camera at `distance` from the origin, looking at it (yaw / pitch as `synthetic.camera_looking_at_origin`), then rolled about
    its viewing axis.  Built in fp64 and rounded to `dtype` at the end; the dictionary of `synthetic.camera`."""
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)
    c = f64([math.sin(yaw) * math.cos(pitch), math.sin(pitch), -math.cos(yaw) * math.cos(pitch)]) * distance
    f = -c / c.norm()
    r = torch.linalg.cross(f64([0.0, 1.0, 0.0]), f)
    r = r / r.norm()
    d = torch.linalg.cross(f, r)
    r, d = math.cos(roll) * r + math.sin(roll) * d, -math.sin(roll) * r + math.cos(roll) * d
    R = torch.stack([r, d, f])                                      # p_cam = R (p_world - c)
    assert float(R.abs().min()) > 0.02, "a pose for these tests has no zero in its rotation"
    w2c = torch.eye(4, dtype=torch.float64)
    w2c[:3, :3] = R.T
    w2c[3, :3] = -(R @ c)
    return _camera_dict(w2c, c, width, height, fx, fy, dtype)


def _camera_dict(w2c, centre, width, height, fx, fy, dtype):
    """The dictionary of `synthetic.camera` for an fp64 world-to-camera matrix (transposed storage), rounded to `dtype` at the end."""
    znear, zfar = 0.01, 100.0
    tanx, tany = 0.5 * width / fx, 0.5 * height / fy
    P = torch.zeros(4, 4, dtype=torch.float64)
    P[0, 0], P[1, 1] = 1.0 / tanx, 1.0 / tany
    P[3, 2] = 1.0
    P[2, 2] = zfar / (zfar - znear)
    P[2, 3] = -(zfar * znear) / (zfar - znear)
    return {"world_to_camera": w2c.to(dtype), "full_projection": (w2c @ P.T).to(dtype), "camera_center": centre.to(dtype), "fx": fx, "fy": fy,
            "cx": width / 2.0, "cy": height / 2.0, "width": width, "height": height, "tanfovx": tanx, "tanfovy": tany}


# yaw, pitch, roll, distance: a plain oblique view, a close-up, a view from behind (yaw above pi / 2)
POSES = {"oblique": (0.5, 0.3, 0.4, 4.0), "close": (-0.7, -0.25, -0.9, 2.2), "behind": (2.4, 0.35, 0.8, 4.5)}

# name -> (scene builder, colour input, scale modifier)
SCENES = {
    "reset-40x24": (lambda: _column_scene(40, 24, 31, False), "shs", 1.0),
    "reset-17x33": (lambda: _column_scene(17, 33, 32, False), "colors_precomp", 1.0),
    "mixed-40x24": (lambda: _column_scene(40, 24, 33, True), "shs", 1.0),
    "mixed-17x33": (lambda: _column_scene(17, 33, 34, True), "colors_precomp", 1.0),
    "clamp-shs": (lambda: _clamp_scene(), "shs", 0.9),
    "clamp-precomp": (lambda: _clamp_scene(), "colors_precomp", 0.9),
}
for _name, (_yaw, _pitch, _roll, _dist) in POSES.items():
    SCENES["pose-" + _name] = (lambda a=(_yaw, _pitch, _roll, _dist): (_special_scene(seed=21)[0], posed_camera(96, 72, 80.0, 78.0, *a)),
                               "shs" if _name == "close" else "colors_precomp", 0.9)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The scene's inputs and its fp64 reference with gradients, computed once and shared (nobody writes to them)."""
    build, colour, mod = SCENES[name]
    params, cam = build()
    W, H = cam["width"], cam["height"]
    cp = torch.rand(params[0].shape[0], 3, generator=torch.Generator().manual_seed(5))
    gen = torch.Generator().manual_seed(9)
    v_color = torch.randn(3, H, W, generator=gen) * 0.1
    v_allmap = torch.randn(7, H, W, generator=gen) * ALLMAP_WEIGHTS[:, None, None]
    r, ref = _oracle(params, cam, BG.double(), mod, colour, v_color.double(), v_allmap.double(), cp)
    return dict(name=name, params=params, cam=cam, mod=mod, colour=colour, cp=cp, v_color=v_color, v_allmap=v_allmap, r=r, ref=ref)


def _statistics(case):
    """The scene's statistics from the oracle alone, printed; the two caps every scene must keep are asserted here."""
    r, cam = case["r"], case["cam"]
    W, H = cam["width"], cam["height"]
    T = 1 - r["allmap"][1].detach()
    visible = int((r["radii"] > 0).sum())
    st = dict(visible=visible, n=int(r["radii"].numel()), lists=(int(r["list_lengths"].min()), int(r["list_lengths"].max())),
              final_T=(float(T.min()), float(T.max())), contributors=(int(r["contributors"].min()), int(r["contributors"].max())),
              pairs_3d=r["pairs_3d"], pairs_lowpass=r["pairs_lowpass"], pairs_clamped=r["pairs_clamped"], stopped=int(r["stopped"].sum()),
              flagged=int(r["flagged"].sum()), excused=int(r["flagged_rows"].sum()), fragile_radii=int(r["pre"]["radius_fragile"].sum()),
              no_median=int(((r["allmap"][5] == 0) & (r["contributors"] > 0)).sum()), pixels=W * H)
    print(f"[{case['name']}] scene: " + ", ".join(f"{k} {v}" for k, v in st.items()))
    assert st["flagged"] <= 0.01 * W * H, f"{st['flagged']} flagged pixels of {W * H}"
    assert st["excused"] <= 0.05 * visible, f"{st['excused']} rows excused of {visible} visible"
    return st


def _conditions(case):
    """What makes the scene the scene it is meant to be; from the oracle alone."""
    name, r = case["name"], case["r"]
    st = _statistics(case)
    if name.startswith("reset"):
        assert st["lists"][0] > 512, "every tile list longer than two staging batches"
        assert 2e-4 < st["final_T"][0] and st["final_T"][1] < 5e-3, "a deep column that does not saturate"
        assert st["stopped"] == 0
        assert st["contributors"][0] >= 600
        assert st["pairs_lowpass"] >= 50 and st["pairs_3d"] >= 100000
    elif name.startswith("mixed"):
        assert 0 < st["stopped"] < st["pixels"], "stopped and unstopped pixels"
        assert st["lists"][1] > 512
        last, spread = r["last"], 0
        for ty in range(0, last.shape[0], 16):
            for tx in range(0, last.shape[1], 16):
                t = last[ty:ty + 16, tx:tx + 16]
                spread = max(spread, int(t.max() - t.min()))
        print(f"[{name}] largest spread of `last` within a tile: {spread}")
        assert spread > 64
    elif name.startswith("clamp"):
        assert st["pairs_clamped"] >= 200
        assert int(r["first_clamped"].sum()) > 0
    else:
        assert st["visible"] > 300
    return st


# ---- CPU: the oracle's statistics, the scenes' conditions, the oracle under a rigid motion -----------------------------------------
def test_oracle_pair_statistics():
    """Three hand-placed surfels over one 16x16 tile and an empty second tile: the counts can be read off."""
    cam = O.synthetic_camera(20, 16, 40.0)
    means = torch.tensor([[-0.2, 0.0, 0.0], [-0.2, 0.0, 0.5], [-0.2, 0.0, 1.0]], dtype=torch.float64)
    scales = torch.tensor([[0.15, 0.15], [0.001, 0.001], [50.0, 50.0]], dtype=torch.float64)
    quats = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * 3, dtype=torch.float64)
    opac = torch.tensor([[1.0], [0.8], [0.9999]], dtype=torch.float64)
    cp = torch.rand(3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    r = SO.render(means, scales, quats, opac, None, 0, cam["world_to_camera"].double(), cam["full_projection"].double(),
                  cam["camera_center"].double(), 20, 16, torch.zeros(3, dtype=torch.float64), colors_precomp=cp)
    assert r["list_lengths"].shape == (1, 2) and int(r["list_lengths"][0, 0]) == 3
    assert r["contributors"].shape == (16, 20) and r["last"].shape == (16, 20)
    assert int(r["contributors"].sum()) == r["pairs_3d"] + r["pairs_lowpass"]
    assert r["pairs_lowpass"] >= 1, "the sub-pixel surfel is seen through the low-pass"
    assert bool((r["last"] >= r["contributors"]).all()) and int(r["last"].max()) <= 3
    # the surfel's centre projects to x = 9.5 - 2 = 7.5, y = 7.5: the four pixels around it see the first surfel at exp(-rho / 2) =
    # exp(-(0.5 / 1.5)^2) = 0.895 (not clamped); the screen-filling last one is clamped wherever it is reached
    assert not bool(r["first_clamped"][7, 7])
    far = r["contributors"] == 1
    assert bool(far.any()) and bool(r["first_clamped"][far].all())
    assert bool((r["last"][:, :16][far[:, :16]] == 3).all()) and bool((r["last"][:, 16:] == 1).all()) and int(r["list_lengths"][0, 1]) == 1
    assert r["pairs_clamped"] >= int(far.sum())
    # front (alpha 0.895, T 0.105), then the clamped 0.99: T (1 - 0.99) = 1e-3 > 1e-4, nobody stops; an opaque pair more would
    assert int(r["stopped"].sum()) == 0
    r2 = SO.render(torch.cat([means, means[2:] + 0.01]), torch.cat([scales, scales[2:]]), torch.cat([quats, quats[2:]]), torch.cat([opac, opac[2:]]),
                   None, 0, cam["world_to_camera"].double(), cam["full_projection"].double(), cam["camera_center"].double(), 20, 16,
                   torch.zeros(3, dtype=torch.float64), colors_precomp=torch.cat([cp, cp[2:]]))
    # two clamped contributors leave T = 1e-4 (1 - 0.99)(1 - 0.99) at best: where the first surfel is in front too, the last one stops
    assert 0 < int(r2["stopped"].sum()) and bool((r2["last"][r2["stopped"]] < 4).all())
    for k in ("render", "allmap", "flagged", "radii"):
        assert torch.equal(r[k], SO.render(means, scales, quats, opac, None, 0, cam["world_to_camera"].double(), cam["full_projection"].double(),
                                           cam["camera_center"].double(), 20, 16, torch.zeros(3, dtype=torch.float64), colors_precomp=cp)[k])


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_reaches_its_path(name):
    _conditions(_case(name))


def _quat_mul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], dim=-1)


def _rotmat_to_quat(M):
    """(w, x, y, z) of a rotation matrix (column-vector convention), fp64, the branch with the largest pivot."""
    m = M.double()
    cands = [(1 + m[0, 0] + m[1, 1] + m[2, 2], lambda s: [s / 4, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s]),
             (1 + m[0, 0] - m[1, 1] - m[2, 2], lambda s: [(m[2, 1] - m[1, 2]) / s, s / 4, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s]),
             (1 - m[0, 0] + m[1, 1] - m[2, 2], lambda s: [(m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, s / 4, (m[1, 2] + m[2, 1]) / s]),
             (1 - m[0, 0] - m[1, 1] + m[2, 2], lambda s: [(m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, s / 4])]
    t, fn = max(cands, key=lambda c: float(c[0]))
    return torch.stack(fn(2 * torch.sqrt(t)))       # s = 4 q_pivot = 2 sqrt(t)


def _moved_into_camera_frame(params, cam, dtype):
    """The scene as the camera `cam` sees it, to be rendered by the identity pose at distance 0."""
    means, scales, quats, opac, shs = params
    V = cam["world_to_camera"].double()
    R, t = V[:3, :3], V[3, :3]
    moved = means.double() @ R + t
    q = _quat_mul(_rotmat_to_quat(R.T), quats.double())            # rotation matrix R^T Rq: axes a_cam = a_world @ R
    ident = _camera_dict(torch.eye(4, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), cam["width"], cam["height"], cam["fx"], cam["fy"],
                         cam["world_to_camera"].dtype)
    return (moved.to(dtype), scales, q.to(dtype), opac, shs), ident


def _render_oracle(params, cam, cp, mod=0.9):
    means, scales, quats, opac, _ = [t.double() for t in params]
    return SO.render(means, scales, quats, opac, None, 0, cam["world_to_camera"].double(), cam["full_projection"].double(),
                     cam["camera_center"].double(), cam["width"], cam["height"], BG.double(), scale_modifier=mod, colors_precomp=cp.double())


# fp64 pose: the two renders differ by the rounding of fp64 alone; 1e-9 leaves seven digits for the conditioning of the sub-pixel
# surfels' intersection.  fp32-rounded pose: R is orthonormal to 6e-8 only, and R -> quaternion -> R projects it back onto a rotation.
@pytest.mark.parametrize("dtype,bound", [(torch.float64, 1e-9), (torch.float32, 5e-6)])
def test_oracle_is_invariant_under_the_rigid_motion_of_a_pose(dtype, bound):
    params = _special_scene(seed=21)[0]
    cp = torch.rand(params[0].shape[0], 3, generator=torch.Generator().manual_seed(5))
    cam = posed_camera(96, 72, 80.0, 78.0, *POSES["oblique"], dtype=dtype)
    a = _render_oracle(params, cam, cp)
    moved, ident = _moved_into_camera_frame(params, cam, torch.float64)
    b = _render_oracle(moved, ident, cp)
    assert torch.equal(a["radii"], b["radii"]) and int((a["radii"] > 0).sum()) > 300
    ok = ~(a["flagged"] | b["flagged"])
    assert int((~ok).sum()) <= 0.01 * ok.numel()
    worst = {"colour": float((a["render"] - b["render"]).abs()[:, ok].max())}
    for ch, label in enumerate(CHANNELS):
        worst[label] = float((a["allmap"][ch] - b["allmap"][ch]).abs()[ok].max())
    print(f"[rigid motion, {dtype}] worst difference per channel: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= bound, worst


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def _forward_errors(tag, color, allmap, r, ok):
    c, a = color.detach().cpu().double(), allmap.detach().cpu().double()
    rc, ra = r["render"].detach(), r["allmap"].detach()
    err = {"colour": (float((c - rc).abs()[:, ok].max()), TOL)}
    for ch, label in enumerate(CHANNELS):
        if ch in (0, 5, 6):      # depth, median: their largest value; distortion: its terms' bound, the alpha
            bound = 1e-5 * (float(ra[1 if ch == 6 else ch].abs().max()) + 1e-12)
        else:
            bound = TOL
        err[label] = (float((a[ch] - ra[ch]).abs()[ok].max()), bound)
    print(f"[{tag}] worst forward error (bound): " + ", ".join(f"{k} {v:.2e} ({b:.1e})" for k, (v, b) in err.items()))
    return err


def _compare(case, det=False):
    """One HIP run of the case against its reference: radii, every forward channel, every gradient."""
    from gspl_amd import _lib as L
    name, r, ref = case["name"], case["r"], case["ref"]
    tag = name + (" deterministic" if det else "")
    old = L.lib().gspl_set_deterministic(1 if det else 0)
    try:
        color, radii, allmap, grads = _run_hip(case["params"], case["cam"], BG, case["mod"], case["colour"], case["v_color"], case["v_allmap"], case["cp"])
    finally:
        L.lib().gspl_set_deterministic(old)
    # (a radius of ~150 px lies within the oracle's 1e-5 relative margin of an integer with probability 3e-3: a few rows of 900)
    fr = r["pre"]["radius_fragile"]
    assert int(fr.sum()) <= 0.01 * fr.numel()
    assert torch.equal(radii.cpu()[~fr], r["radii"][~fr]), "radii"
    ok = ~r["flagged"]
    err = _forward_errors(tag, color, allmap, r, ok)
    excused = r["flagged_rows"].numpy()
    ratios = {}
    for k in ref:
        g, rf = grads[k].detach().cpu().double().reshape(ref[k].shape[0], -1).numpy(), ref[k].detach().reshape(ref[k].shape[0], -1).numpy()
        rel = np.abs(g - rf) / (np.abs(rf) + np.sqrt(np.mean(rf * rf)) + 1e-30)
        ratios[k] = (float(rel[~excused].max()), float(np.median(rel)), int(((rel > 2e-3).any(1) & ~excused).sum()))
    print(f"[{tag}] gradient ratio |got - ref| / (|ref| + rms), worst off the excused rows / median / rows beyond 2e-3: " +
          ", ".join(f"{k} {w:.2e} / {m:.1e} / {b}" for k, (w, m, b) in ratios.items()))
    for k, (v, b) in err.items():
        assert v <= b, f"{tag}: {k} off by {v:.3e} (bound {b:.1e})"
    for k in ref:
        assert bool(torch.isfinite(grads[k]).all()), k
        _grad_check(f"{tag} {k}", grads[k], ref[k], excused)
    return color, radii, allmap, grads


@gpu
@pytest.mark.parametrize("name,det", [("reset-40x24", False), ("reset-17x33", False), ("reset-17x33", True)])
def test_deep_unsaturated_column_after_a_reset(name, det):
    case = _case(name)
    _conditions(case)
    assert int(case["r"]["list_lengths"].sum()) > 4500          # the deterministic mode's rows, one per list entry (4954 and 4937)
    _compare(case, det)


@gpu
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", ["mixed-40x24", "mixed-17x33"])
def test_long_lists_whose_pixels_stop_at_different_positions(name, det):
    case = _case(name)
    _conditions(case)
    _compare(case, det)


@gpu
@pytest.mark.parametrize("name", ["clamp-shs", "clamp-precomp"])
def test_alpha_clamp_and_its_straight_through_backward(name):
    case = _case(name)
    _conditions(case)
    color, radii, allmap, grads = _compare(case)
    first = case["r"]["first_clamped"] & ~case["r"]["flagged"]
    assert int(first.sum()) > 0
    lowest = float(allmap[1].cpu()[first].min())
    print(f"[{name}] {int(first.sum())} pixels clamped by their first contributor, lowest alpha {lowest:.6f}")
    assert lowest >= 0.99 - TOL


@gpu
@pytest.mark.parametrize("name", ["pose-" + k for k in POSES])
def test_rotated_view_against_fp64_oracle(name):
    case = _case(name)
    _conditions(case)
    _compare(case)


@gpu
def test_rotated_view_equals_the_moved_scene_under_the_identity_pose():
    """The two HIP renders of the rigid-motion pair, against each other (the oracle only says which pixels hold a fragile decision)."""
    params = _special_scene(seed=21)[0]
    cp = torch.rand(params[0].shape[0], 3, generator=torch.Generator().manual_seed(5))
    cam = posed_camera(96, 72, 80.0, 78.0, *POSES["oblique"])
    moved, ident = _moved_into_camera_frame(params, cam, torch.float32)
    zc, za = torch.zeros(3, 72, 96), torch.zeros(7, 72, 96)
    ca, ra, aa, _ = _run_hip(params, cam, BG, 0.9, "colors_precomp", zc, za, cp)
    cb, rb, ab, _ = _run_hip(moved, ident, BG, 0.9, "colors_precomp", zc, za, cp)
    oa, ob = _render_oracle(params, cam, cp), _render_oracle(moved, ident, cp)
    ok = ~(oa["flagged"] | ob["flagged"])
    assert int((~ok).sum()) <= 0.02 * ok.numel()
    fr = oa["pre"]["radius_fragile"] | ob["pre"]["radius_fragile"]
    assert torch.equal(ra.cpu()[~fr], rb.cpu()[~fr]) and int((ra > 0).sum()) > 300
    ca, cb, aa, ab = [t.detach().cpu().double() for t in (ca, cb, aa, ab)]
    worst = {"colour": (float((ca - cb).abs()[:, ok].max()), 2 * TOL)}
    for ch, label in enumerate(CHANNELS):
        scale = float(oa["allmap"][1 if ch == 6 else ch].abs().max()) + 1e-12
        worst[label] = (float((aa[ch] - ab[ch]).abs()[ok].max()), 2 * (1e-5 * scale if ch in (0, 5, 6) else TOL))
    print("[rigid motion, HIP] worst difference (bound): " + ", ".join(f"{k} {v:.2e} ({b:.1e})" for k, (v, b) in worst.items()))
    for k, (v, b) in worst.items():
        assert v <= b, f"{k}: {v:.3e} (bound {b:.1e})"


@gpu
@pytest.mark.parametrize("fused", [False, True])
def test_renderer_plugin_under_a_rotated_view(fused):
    """`HipVanilla2DGSRenderer` hands the camera's matrices to the op as they are: its maps are the op's for the same matrices."""
    from fakes import FakeCamera, FakeGaussianModel
    from gspl_amd import ops
    from gspl_amd.renderers import HipVanilla2DGSRenderer
    dev = torch.device("cuda:0")
    case = _case("pose-behind")
    cam = case["cam"]
    means, scales, quats, opac, shs = [t.to(dev) for t in case["params"]]
    model = FakeGaussianModel(means, torch.cat([scales, torch.full((scales.shape[0], 1), 1e-3, device=dev)], dim=1), quats, opac, shs)
    out = HipVanilla2DGSRenderer(depth_ratio=0.0, fused_maps=fused)(FakeCamera(cam, dev), model, BG.to(dev), scaling_modifier=case["mod"])
    with torch.no_grad():
        color, radii, allmap = ops.SurfelGaussianRasterizer(_settings(cam, BG, case["mod"], dev))(
            means3D=means, means2D=torch.zeros_like(means), opacities=opac, scales=scales, rotations=quats, shs=shs)
    assert torch.equal(out["render"], color) and torch.equal(out["radii"], radii)
    assert torch.equal(out["rend_alpha"], allmap[1:2]) and torch.equal(out["rend_dist"], allmap[6:7])
    V3 = cam["world_to_camera"][:3, :3].to(dev)
    normal = (allmap[2:5].permute(1, 2, 0) @ V3.T).permute(2, 0, 1)
    depth = torch.nan_to_num(allmap[0:1] / allmap[1:2], 0, 0)
    # the fused maps are one HIP kernel on the same fp32 values: a few roundings of a unit vector and of depth / alpha
    tol_n, tol_d = (0.0, 0.0) if not fused else (1e-6, 1e-6 * float(depth.abs().max()))
    dn, dd = float((out["rend_normal"] - normal).abs().max()), float((out["surf_depth"] - depth).abs().max())
    print(f"[renderer, fused_maps={fused}] rend_normal off by {dn:.2e}, surf_depth by {dd:.2e}")
    assert dn <= tol_n and dd <= tol_d
    # ... and the op's own normals are the oracle's under this pose (a transposed view matrix would show here): three components
    # within TOL each, rotated: within sqrt(3) TOL
    ok = ~case["r"]["flagged"].to(dev)
    ref_normal = (case["r"]["allmap"][2:5].detach().permute(1, 2, 0) @ cam["world_to_camera"][:3, :3].double().T).permute(2, 0, 1)
    assert float((out["rend_normal"].double().cpu() - ref_normal).abs()[:, ok.cpu()].max()) <= 2 * TOL

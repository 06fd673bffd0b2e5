"""The two per-splat preprocess kernels with the camera INSIDE the cloud, pinned to the fp64 oracle one cotangent group at a time.

`gspl_project_fwd/bwd` (csrc/projection.hip, gsplat convention) and `gspl_inria_preprocess_fwd/bwd` (csrc/inria.hip, Inria convention)
share the EWA code of csrc/gspl_device.h.  The calibrated scenes of test_hip_parity.py look at a cloud from outside: the 1.3 tan(fov) clamp
of the Jacobian is active on one visible splat-view in a thousand there, nothing is behind the camera or near a near plane, and with all
cotangents summed the screen-position path swamps the conic path, so a backward with the WRONG clamp derivative (the Inria rule in the
gsplat kernel or the other way round) passes every bar of those tests.  Here:

Scene: `O.synthetic_scene(4096, seed=5)`, scales x 12, a 320 x 208 image, fx, fy = 300, 295, the camera at distance 0.7 from the centre
of the cloud and rotated by 0.6 rad about normalize(randn(3, Generator(5))) (the construction of tools/fuzz_parity.random_case).  Class
counts of the fp64 oracle (asserted below: every class holds at least 150 rows):

    quantity                    gsplat   Inria
    visible                       1963    1796
    visible, no clamp              793     792
    visible, clamp in x only       235     216
    visible, clamp in y only       480     444
    visible, clamp in both         455     344
    behind the camera (z < 0): 853;  0 <= z < 0.01: 15;  0.01 <= z < 0.2: 321 (108 visible under gsplat's near plane, none under Inria's 0.2)

Rows ON a threshold are left out, at most 4 per case (asserted): view-space z within 1e-5 relative of a near or far plane in use, |x/z| or
|y/z| within 1e-5 relative of its clamp limit, a GPU radius that differs from the oracle's.  On the CPU the first two counts are 0 for
every case of this module (asserted by the calibration test).

Classes: the four clamp states of the table; under gsplat's near plane the kept rows with z < 0.2 (108) are a fifth class, `near_band`:
they are one to two orders of magnitude larger than the rest and would otherwise BE the rms of the classes they fall in.  Every kept row
is in a class for the forward checks and for every cotangent group but one: under the STRUCTURED conic cotangent the rows whose 2D
covariance has lambda_max / lambda_min > 16 (`KAPPA_MAX`; 176 of the 1963 visible rows, 153 of Inria's 1796) are in no class.  Why: that
cotangent is a product built to cancel against the conic (-conic G conic = V), and what the fp32 ORACLE makes of it depends on the
conditioning: with all rows it misses on `v_scales` (2.9e-4 in the both-clamped class), with kappa <= 64 it sits at 4.8e-5, on the bound,
and with kappa <= 16 at 1.5e-5 (means 2.3e-6, quats 5.3e-6).  The cut is made on the oracle's fp64 conic, never on the kernel's output;
every class keeps at least 150 rows under it (asserted).

Gradient bar: `assert_close_scaled(rel=1e-4, frac_ok=1.0)` PER CLASS (each class is scaled by its own rms: the near-camera rows dominate
a global rms) and PER COTANGENT GROUP (with a conic-only cotangent the swapped clamp rule moves almost every clamped row by more than
1e-4; summed with the screen-position cotangent it moves `v_means` by a median of 8e-11).  Groups: `v_means2d`; `v_depths`;
`v_compensations`; `v_conics` = 0.1 randn; `v_conics` structured, G = -Sigma V Sigma with Sigma the oracle's fp64 2D covariance (low-pass
included) and V a random symmetric matrix of unit scale: the shape and magnitude compositing hands the kernel; (Inria) `v_colors`.

Calibration (`test_fp32_oracle_holds_half_the_bar`, no GPU): the bar comes from the reference, not from the kernel.  The oracle is
evaluated in fp32 and in fp64 for every (case, group, output, class) the GPU tests assert and must agree within 5e-5 under the same
scaling: half the bar, the other half is left for a different but equally valid order of fp32 operations.  A combination the fp32
oracle does not hold is NOT asserted on the GPU; it is listed in `NOT_FP32` with its measured value.  torch's fp32 sums differ between
host CPUs, so the list keeps a factor of two from the bound on both sides: every combination measured beyond 2.5e-5 is listed (nothing
asserted was above 2.5e-5 where the list was written, and must be within 5e-5 anywhere), and a listed one must still be beyond 1e-5
wherever the test runs (the smallest listed value is 4.8e-5).  The 1e-4 is never loosened.  `v_compensations` cannot be held in this scene
(every splat is tens of pixels wide, the compensation is 1 - O(eps2d / lambda)); it is held on `NARROW`, the same cloud with scales x 0.25:
600 visible splats about a pixel wide, compensations 0.2 ... 0.75, fp32 oracle within 8e-6.

Mutations (each fails the new tests named; "old": the tests of test_hip_parity.py, test_camera_models.py and test_locked_parity.py — its
1080p cases left out — that fail under the same mutation; mutations 5 and 6 were applied together with others, see the note):
    1 `ewa_bwd<true>` -> `<false>` in project_bwd_kernel    every pinhole gsplat test but the narrow one (clamped classes)
                                                            old: test_smoke_scene_locked[gsplat], test_trained_scene_shaped_workload_locked[S-smoke-surfaces-gsplat]
    2 `ewa_bwd<false>` -> `<true>` in the Inria backward    test_inria_preprocess_inside_the_cloud, test_inria_preprocess_variants[*]
                                                            old: test_smoke_scene_locked[vanilla], test_trained_scene_shaped_workload_locked[S-smoke-surfaces-vanilla]
    3 `vz += vty * ctx.uy` dropped                          every pinhole gsplat test but the narrow one (clamp_y, clamp_xy, near_band)
                                                            old: test_smoke_scene_locked[gsplat]
    4 `rf <= radius_clip` -> `<`                            test_gsplat_projection_argument_sweep[clip_equal]                 old: none
    5 far_plane ignored                                     test_gsplat_projection_argument_sweep[far1.2]                     old: not separated
    6 Inria near plane 0.2 -> 0.01                          test_inria_preprocess_inside_the_cloud, test_inria_preprocess_variants[*]   old: none
    7 `vs[j] *= scale_modifier` dropped (both kernels)      test_gsplat_projection_argument_sweep[smod0.5, smod2], test_inria_preprocess_variants[smod0.5, smod2]
                                                            old: test_inria_api_precomputed_cov3d_and_colors_and_scale_modifier
    8 strided v_conics read with the dense stride           test_gsplat_backward_reads_strided_cotangents
                                                            old: test_end_to_end_gsplat_api, three test_locked_parity.py cases on the gsplat smoke scene
Note: 5 was applied together with 2, 4 and 8 (far1.2 is the only new failure none of those three causes alone; the old modules of that
combination were not run to the end), 6 together with 3 and 4 (the Inria failures are 6's: 3 and 4 alone fail gsplat tests only; the only
old failure of that combination is 3's).  The clip of `clip_equal` is a radius that a dozen splats have: with fewer than five, `<` for `<=`
hides among the rows on a threshold.

CALIBRATION (fp32 oracle against fp64 oracle, worst element / (|ref| + rms of the class), maximum over the classes, on the machine the
list was written on; the figures move from one host CPU to the next, e.g. 5.4e-5 here and 1.5e-5 there for one fisheye class):
    gsplat              xy/means 3.3e-06               depth/means 4.5e-08            comp/means 3.2e-01             comp/scales 4.1e-02            comp/quats 1.5e-01
                        conic_rand/means 9.3e-06       conic_rand/scales 5.5e-06      conic_rand/quats 1.7e-05       conic_struct/means 2.3e-06     conic_struct/scales 1.5e-05
                        conic_struct/quats 5.3e-06
    gsplat/C3           xy/means 5.7e-06               depth/means 1.3e-07            comp/means 5.5e-02             comp/scales 4.0e-03            comp/quats 3.5e-03
                        conic_rand/means 1.7e-05       conic_rand/scales 1.2e-05      conic_rand/quats 4.8e-05       conic_struct/means 1.9e-06     conic_struct/scales 6.3e-06
                        conic_struct/quats 4.2e-06
    inria               xy/means 4.6e-07               conic_rand/means 9.2e-06       conic_rand/scales 4.1e-06      conic_rand/quats 1.7e-05       conic_struct/means 2.2e-06
                        conic_struct/scales 1.5e-05    conic_struct/quats 5.2e-06     color/means 7.2e-07            color/shs 8.9e-07
    gsplat/narrow       comp/means 3.0e-06             comp/scales 1.1e-06            comp/quats 8.0e-06
    gsplat/near0.2      conic_struct/means 2.3e-06     conic_struct/scales 1.5e-05    conic_struct/quats 5.3e-06
    gsplat/near0.5      conic_struct/means 1.2e-06     conic_struct/scales 7.7e-06    conic_struct/quats 2.5e-06
    gsplat/far1.2       conic_struct/means 2.3e-06     conic_struct/scales 1.4e-05    conic_struct/quats 4.8e-06
    gsplat/clip_equal   conic_struct/means 2.3e-06     conic_struct/scales 1.5e-05    conic_struct/quats 5.0e-06
    gsplat/clip_between conic_struct/means 2.3e-06     conic_struct/scales 1.5e-05    conic_struct/quats 5.0e-06
    gsplat/eps0.1       conic_struct/means 1.7e-06     conic_struct/scales 6.4e-06    conic_struct/quats 4.4e-06
    gsplat/smod0.5      conic_struct/means 1.5e-06     conic_struct/scales 4.6e-06    conic_struct/quats 2.7e-06
    gsplat/smod2        conic_struct/means 1.9e-06     conic_struct/scales 7.8e-06    conic_struct/quats 5.4e-06
    gsplat/ortho        xy/means 9.8e-08               depth/means 4.5e-08            comp/scales 2.8e-03            comp/quats 1.2e-02             conic_rand/scales 8.9e-06
                        conic_rand/quats 1.1e-05       conic_struct/scales 1.1e-05    conic_struct/quats 7.2e-06
    gsplat/fisheye      xy/means 5.9e-07               depth/means 4.5e-08            comp/means 3.9e-03             comp/scales 4.9e-04            comp/quats 3.6e-03
                        conic_rand/means 2.9e-03       conic_rand/scales 1.3e-05      conic_rand/quats 1.0e-05       conic_struct/means 3.0e-03     conic_struct/scales 5.9e-06
                        conic_struct/quats 7.2e-06
    inria/smod0.5       conic_rand/means 7.4e-06       conic_rand/scales 5.3e-06      conic_rand/quats 9.0e-06       color/means 6.4e-07            color/shs 8.9e-07
    inria/smod2         conic_rand/means 5.7e-06       conic_rand/scales 4.6e-06      conic_rand/quats 2.0e-05       color/means 7.8e-07            color/shs 8.9e-07
    inria/cov_pre       conic_rand/means 1.9e-05       conic_rand/cov6 2.4e-05        color/means 7.2e-07            color/shs 8.9e-07
    inria/colors_pre    conic_rand/means 9.2e-06       conic_rand/scales 4.1e-06      conic_rand/quats 1.7e-05
"""
import functools
import math
from dataclasses import dataclass, replace

import numpy as np
import pytest
import torch

from oracle import gsplat_oracle as O
from hip_helpers import assert_close_scaled, cov2d_condition
from private_pool import private_memory_pool  # noqa: F401   (autouse: older tests depend on allocator addresses)

N, W, H, FX, FY = 4096, 320, 208, 300.0, 295.0
REL, HALF_BAR = 1e-4, 5e-5
LISTED_FLOOR = 1e-5        # a combination listed in NOT_FP32 must be beyond this on any host (listed where written: beyond 2.5e-5)
MAX_LEFT_OUT = 4           # rows on a threshold, per case: 0.1 %
MIN_CLASS_ROWS = 150
KAPPA_MAX = 16.0           # structured conic cotangent only: rows whose 2D covariance is worse conditioned are in no class (module docstring)
NEAR_BAND = 0.2            # gsplat: the rows between its near plane and Inria's are a class of their own
N_PLANTED = 48             # fisheye: means planted next to the optical axis
POSES = ((0.6, 5, 0.7), (-0.9, 6, 0.4), (1.4, 7, 1.0))      # (angle, seed of the axis, distance): all inside the cloud (|means| <= 1.3)


@dataclass(frozen=True)
class Case:
    api: str = "gsplat"            # "gsplat" | "inria"
    poses: tuple = (0,)
    near: float = 0.01             # gsplat only (Inria's 0.2 is a constant of the kernel)
    far: float = 1e10
    clip: str = ""                 # "": none; "equal": a radius a dozen visible splats have EXACTLY; "between": that + 0.5
    eps2d: float = 0.3
    smod: float = 1.0
    model: str = "pinhole"
    cov_pre: bool = False          # Inria: cov3D_precomp instead of scales + rotations
    colors_pre: bool = False       # Inria: colors_precomp instead of SH coefficients
    scale_mul: float = 12.0        # the scene's scales; 0.25: splats about a pixel wide, where the compensation is not 1


GSPLAT, INRIA = Case(), Case(api="inria")
GSPLAT_C3 = Case(poses=(0, 1, 2))
NARROW = Case(scale_mul=0.25)
SWEEP = {
    "near0.2": replace(GSPLAT, near=0.2), "near0.5": replace(GSPLAT, near=0.5), "far1.2": replace(GSPLAT, far=1.2),
    "clip_equal": replace(GSPLAT, clip="equal"), "clip_between": replace(GSPLAT, clip="between"),
    "eps0.1": replace(GSPLAT, eps2d=0.1), "smod0.5": replace(GSPLAT, smod=0.5), "smod2": replace(GSPLAT, smod=2.0),
}
MODELS = {"ortho": replace(GSPLAT, model="ortho"), "fisheye": replace(GSPLAT, model="fisheye")}
INRIA_VARIANTS = {"smod0.5": replace(INRIA, smod=0.5), "smod2": replace(INRIA, smod=2.0), "cov_pre": replace(INRIA, cov_pre=True),
                  "colors_pre": replace(INRIA, colors_pre=True)}
SWEEP_GROUP = "conic_struct"       # the one gradient group of the argument sweep: the one the clamp rule shows in
INRIA_VARIANT_GROUPS = ("conic_rand", "color")

# (case, group, output, class) -> fp32 oracle against fp64 oracle, measured: beyond 5e-5, so not asserted on the GPU
NOT_FP32 = {
    # the compensation sqrt(det0 / det1): every splat of this scene is tens of pixels wide, det0 / det1 = 1 - O(eps2d / lambda), and its
    # derivative is the difference of two terms that agree to eps2d / lambda: eps32 lambda / eps2d of the element itself in ANY fp32 evaluation
    # (held on the pixel-wide splats of NARROW instead)
    ('gsplat', 'comp', 'means', 'inside'): 1.3e-03,
    ('gsplat', 'comp', 'means', 'clamp_x'): 1.9e-03,
    ('gsplat', 'comp', 'means', 'clamp_y'): 2.0e-03,
    ('gsplat', 'comp', 'means', 'clamp_xy'): 1.5e-02,
    ('gsplat', 'comp', 'means', 'near_band'): 3.2e-01,
    ('gsplat', 'comp', 'scales', 'inside'): 2.2e-04,
    ('gsplat', 'comp', 'scales', 'clamp_x'): 6.5e-04,
    ('gsplat', 'comp', 'scales', 'clamp_y'): 3.3e-04,
    ('gsplat', 'comp', 'scales', 'clamp_xy'): 1.9e-03,
    ('gsplat', 'comp', 'scales', 'near_band'): 4.1e-02,
    ('gsplat', 'comp', 'quats', 'inside'): 2.8e-03,
    ('gsplat', 'comp', 'quats', 'clamp_x'): 1.6e-03,
    ('gsplat', 'comp', 'quats', 'clamp_y'): 8.4e-04,
    ('gsplat', 'comp', 'quats', 'clamp_xy'): 3.9e-03,
    ('gsplat', 'comp', 'quats', 'near_band'): 1.5e-01,
    ('gsplat/C3', 'comp', 'means', 'inside'): 3.9e-04,
    ('gsplat/C3', 'comp', 'means', 'clamped'): 5.5e-02,
    ('gsplat/C3', 'comp', 'scales', 'inside'): 1.8e-04,
    ('gsplat/C3', 'comp', 'scales', 'clamped'): 4.0e-03,
    ('gsplat/C3', 'comp', 'quats', 'inside'): 2.0e-04,
    ('gsplat/C3', 'comp', 'quats', 'clamped'): 3.5e-03,
    ('gsplat/ortho', 'comp', 'scales', 'visible'): 2.8e-03,
    ('gsplat/ortho', 'comp', 'quats', 'visible'): 1.2e-02,
    ('gsplat/fisheye', 'comp', 'means', 'near_axis'): 3.9e-03,
    ('gsplat/fisheye', 'comp', 'means', 'wide_angle'): 3.2e-03,
    ('gsplat/fisheye', 'comp', 'means', 'between'): 1.6e-03,
    ('gsplat/fisheye', 'comp', 'scales', 'near_axis'): 3.7e-04,
    ('gsplat/fisheye', 'comp', 'scales', 'wide_angle'): 3.3e-04,
    ('gsplat/fisheye', 'comp', 'scales', 'between'): 4.9e-04,
    ('gsplat/fisheye', 'comp', 'quats', 'near_axis'): 1.3e-03,
    ('gsplat/fisheye', 'comp', 'quats', 'wide_angle'): 3.6e-03,
    ('gsplat/fisheye', 'comp', 'quats', 'between'): 1.1e-03,
    # the fisheye Jacobian's d/d(mean) next to the axis: quotients by r and r^2 + eps of nearly cancelling terms
    ('gsplat/fisheye', 'conic_rand', 'means', 'near_axis'): 2.9e-03,
    ('gsplat/fisheye', 'conic_struct', 'means', 'near_axis'): 3.0e-03,
    # three cameras' sums under the random conic cotangent, all rows: within a factor of two of half the bar
    ('gsplat/C3', 'conic_rand', 'quats', 'clamped'): 4.8e-05,
}


# ---------------------------------------------------------------------------------------------
# scene, cameras, cotangents
# ---------------------------------------------------------------------------------------------
def _camera(pose):
    """`tools/fuzz_parity.random_case`'s rotated camera: rotation by `angle` about a random axis THROUGH THE SCENE CENTRE."""
    angle, seed, distance = POSES[pose]
    cam = O.synthetic_camera(W, H, FX, FY, distance=distance)
    ax = torch.nn.functional.normalize(torch.randn(3, generator=torch.Generator().manual_seed(seed)), dim=0)
    Kx = torch.tensor([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = torch.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)
    w2c = cam["world_to_camera"].clone()
    w2c[:3, :3] = R.T      # transposed storage: rows 0-2 hold R^T, row 3 the translation
    P = torch.linalg.inv(cam["world_to_camera"]) @ cam["full_projection"]
    cam["world_to_camera"] = w2c
    cam["full_projection"] = w2c @ P
    cam["camera_center"] = torch.linalg.inv(w2c)[3, :3]
    return cam


@functools.lru_cache(None)
def _params(case):
    """fp32 parameters of the case, as both sides read them."""
    means, scales, quats, _, shs = O.synthetic_scene(N, seed=5)
    scales = scales * case.scale_mul
    if case.model == "fisheye":
        # a few dozen means next to the optical axis: camera-space (x, y) = (1e-5 ... 9e-4) z
        g = torch.Generator().manual_seed(11)
        w2c = _camera(case.poses[0])["world_to_camera"].double()
        z = 0.05 + 1.2 * torch.rand(N_PLANTED, generator=g, dtype=torch.float64)
        r = z * 10 ** (-5 + 1.95 * torch.rand(N_PLANTED, generator=g, dtype=torch.float64))
        phi = 2 * math.pi * torch.rand(N_PLANTED, generator=g, dtype=torch.float64)
        pc = torch.stack([r * torch.cos(phi), r * torch.sin(phi), z], dim=-1)
        means = means.clone()
        means[:N_PLANTED] = ((pc - w2c[3, :3]) @ torch.linalg.inv(w2c[:3, :3])).float()
    p = {"means": means, "scales": scales, "quats": quats}
    if case.api == "inria":
        p["shs"] = shs
    if case.cov_pre:
        S = O.cov3d_from_scale_rot(scales.double(), 1.0, quats.double()).reshape(N, 9)
        p["cov6"] = S[:, [0, 1, 2, 4, 5, 8]].float()
        del p["scales"], p["quats"]
    if case.colors_pre:
        p["colors"] = torch.rand(N, 3, generator=torch.Generator().manual_seed(12))
        del p["shs"]
    return p


class _Ref:
    """One oracle evaluation (graph kept): outputs [C, N, ...], the decisions, and gradients per cotangent group."""

    def __init__(self, case, dtype):
        self.case, self.dtype = case, dtype
        self.leaves = {k: v.to(dtype).requires_grad_(True) for k, v in _params(case).items()}
        lv = self.leaves
        outs = {k: [] for k in ("xy", "depth", "conic", "comp", "color")}
        self.radii, self.tiles, self.keep, self.pc, self.raw_color = [], [], [], [], []
        for pose in case.poses:
            cam = _camera(pose)
            w2c = cam["world_to_camera"].to(dtype)
            pc = (lv["means"].detach() @ w2c[:3, :3] + w2c[3, :3])
            self.pc.append(pc.numpy().astype(np.float64))
            if case.api == "gsplat":
                xy, dep, rad, con, comp, tiles, _, mask, _, _ = O.project_gaussians(
                    lv["means"], lv["scales"], case.smod, lv["quats"], w2c, FX, FY, cam["cx"], cam["cy"], H, W,
                    min_depth=case.near, eps2d=case.eps2d, camera_model=case.model)
                # the oracle has neither a far plane nor a radius clip: a mask on its outputs
                keep = mask & (pc[:, 2] <= case.far)
                if case.clip:
                    keep = keep & ~(rad.to(dtype) <= self.clip_value(rad, mask))
                col = None
            else:
                xy, dep, rad, con, mask = O.inria_preprocess(
                    lv["means"], lv.get("scales"), case.smod, lv.get("quats"), w2c, cam["full_projection"].to(dtype),
                    cam["tanfovx"], cam["tanfovy"], H, W, cov3d_precomp=lv.get("cov6"))
                keep, comp, tiles = mask, None, None
                col = lv["colors"] if case.colors_pre else O.sh_colors(3, lv["shs"], lv["means"], cam["camera_center"].to(dtype), detach_dirs=False)
                self.raw_color.append(col.detach().numpy().astype(np.float64))
            zero = torch.zeros((), dtype=dtype)
            for k, v in (("xy", xy), ("depth", dep), ("conic", con), ("comp", comp), ("color", col)):
                if v is not None:
                    outs[k].append(torch.where(keep.reshape((-1,) + (1,) * (v.dim() - 1)), v, zero))
            self.radii.append(torch.where(keep, rad, torch.zeros((), dtype=torch.int32)).numpy())
            self.tiles.append(None if tiles is None else torch.where(keep, tiles, torch.zeros((), dtype=torch.int32)).numpy())
            self.keep.append(keep.numpy())
        self.outs = {k: torch.stack(v) for k, v in outs.items() if v}
        self._grads = {}

    def clip_value(self, rad, mask):
        if self.dtype != torch.float64:
            return _ref(self.case, torch.float64).clip
        vis = rad.numpy()[mask.numpy()]
        lo, hi = np.quantile(vis, [0.3, 0.7])
        vals, counts = np.unique(vis[(vis >= lo) & (vis <= hi)], return_counts=True)      # the most frequent radius of the middle of the range
        self.clip = float(vals[np.argmax(counts)]) + (0.5 if self.case.clip == "between" else 0.0)
        return self.clip

    def out(self, name):
        return self.outs[name].detach().numpy().astype(np.float64)

    def grads(self, group):
        """{leaf: dL/dleaf, float64 numpy} for L = sum over the group's outputs of <output, cotangent>, summed over the cameras."""
        if group not in self._grads:
            cots = _cotangents(self.case)[group]
            names = list(self.leaves)
            g = torch.autograd.grad([self.outs[k] for k in cots], [self.leaves[n] for n in names],
                                    [v.to(self.dtype) for v in cots.values()], retain_graph=True, allow_unused=True)
            self._grads[group] = {n: (np.zeros(tuple(self.leaves[n].shape)) if t is None else t.numpy().astype(np.float64)) for n, t in zip(names, g)}
        return self._grads[group]


@functools.lru_cache(None)
def _ref(case, dtype=torch.float64):
    return _Ref(case, dtype)


def _groups(case):
    if case.api == "gsplat":
        return ("xy", "depth", "comp", "conic_rand", "conic_struct")
    return ("xy", "conic_rand", "conic_struct", "color")


@functools.lru_cache(None)
def _cotangents(case):
    """{group: {output name: cotangent [C, N, ...] float64}}; the structured conic cotangent comes from the fp64 oracle's conics."""
    C = len(case.poses)
    g = torch.Generator().manual_seed(20 + C)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    cots = {"xy": {"xy": rn(C, N, 2)}, "conic_rand": {"conic": 0.1 * rn(C, N, 3)}}
    con = torch.from_numpy(_ref(case).out("conic"))
    A, B, Cc = con.unbind(-1)
    det = A * Cc - B * B
    ok = det > 0
    det = torch.where(ok, det, torch.ones_like(det))
    sa, sb, sc = Cc / det, -B / det, A / det            # Sigma = conic^-1 = the 2D covariance with the low-pass added
    va, vb, vc = rn(C, N), rn(C, N), rn(C, N)           # V symmetric, unit scale
    # G = -Sigma V Sigma; the cotangent of the stored triple (a, b, c) is (G00, 2 G01, G11): b is ONE parameter, as compositing hands it over
    m00, m01 = va * sa + vb * sb, va * sb + vb * sc     # V Sigma
    m10, m11 = vb * sa + vc * sb, vb * sb + vc * sc
    g00, g01, g11 = -(sa * m00 + sb * m10), -(sa * m01 + sb * m11), -(sb * m01 + sc * m11)
    zero = torch.zeros_like(g00)
    cots["conic_struct"] = {"conic": torch.stack([torch.where(ok, g00, zero), torch.where(ok, 2 * g01, zero), torch.where(ok, g11, zero)], dim=-1)}
    if case.api == "gsplat":
        cots["depth"] = {"depth": rn(C, N)}
        cots["comp"] = {"comp": rn(C, N)}
    else:
        cots["color"] = {"color": rn(C, N, 3)}
    # every cotangent is an fp32 number: the fp64 oracle is handed exactly what the kernel is handed (the structured one is a product
    # that nearly cancels in the chain behind it: its own rounding to fp32 would otherwise count as the kernel's error)
    return {g: {k: v.float().double() for k, v in d.items()} for g, d in cots.items()}


def _outputs_of(case):
    return tuple(_params(case))


# ---------------------------------------------------------------------------------------------
# classes and rows on a threshold
# ---------------------------------------------------------------------------------------------
def _limits():
    return 1.3 * (0.5 * W / FX), 1.3 * (0.5 * H / FY)


def _threshold_rows(case, ci=0):
    """(z on a plane in use, |x/z| or |y/z| on its clamp limit) within 1e-5 relative — bool [N] each, from the fp64 oracle."""
    pc = _ref(case).pc[ci]
    z = pc[:, 2]
    planes = [0.2] if case.api == "inria" else [case.near] + ([case.far] if case.far < 1e9 else [])
    on_plane = np.zeros(N, bool)
    for p in planes:
        on_plane |= np.abs(z - p) <= 1e-5 * p
    on_limit = np.zeros(N, bool)
    if case.model == "pinhole":
        with np.errstate(divide="ignore", invalid="ignore"):
            for k, lim in enumerate(_limits()):
                on_limit |= np.abs(np.abs(pc[:, k] / z) - lim) <= 1e-5 * lim
    return on_plane, on_limit


def _classes(case, ci=0):
    """{class name: bool [N]} over the rows the fp64 oracle keeps in camera `ci`."""
    r = _ref(case)
    pc, keep = r.pc[ci], r.keep[ci]
    with np.errstate(divide="ignore", invalid="ignore"):
        ux, uy = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
    if case.model == "pinhole":
        limx, limy = _limits()
        cx, cy = np.abs(ux) > limx, np.abs(uy) > limy
        near = pc[:, 2] < NEAR_BAND
        far = keep & ~near
        cls = {"inside": far & ~cx & ~cy, "clamp_x": far & cx & ~cy, "clamp_y": far & ~cx & cy, "clamp_xy": far & cx & cy}
        cls["near_band"] = keep & near
        return {k: v for k, v in cls.items() if v.any() or k == "inside"}
    if case.model == "fisheye":
        rr = np.hypot(pc[:, 0], pc[:, 1])
        axis, wide = rr < 1e-3 * pc[:, 2], np.arctan2(rr, pc[:, 2]) > math.radians(60.0)
        return {"near_axis": keep & axis, "wide_angle": keep & wide, "between": keep & ~axis & ~wide}
    return {"visible": keep}


def _ill_conditioned(case, ci=0):
    """bool [N]: kept rows whose fp64 2D covariance (from the oracle's conic) has lambda_max / lambda_min > KAPPA_MAX."""
    r = _ref(case)
    return r.keep[ci] & (cov2d_condition(r.out("conic")[ci]) > KAPPA_MAX)


def _union_classes(case):
    """Classes of a gradient that is summed over the cameras: rows some camera sees, split by whether any seeing camera clamps them."""
    seen, clamped = np.zeros(N, bool), np.zeros(N, bool)
    for ci in range(len(case.poses)):
        c = _classes(case, ci)
        seen |= _ref(case).keep[ci]
        clamped |= _ref(case).keep[ci] & ~c["inside"]
    return {"inside": seen & ~clamped, "clamped": seen & clamped}


def _grad_classes(case, group=None):
    """Classes of one cotangent group's gradients: under the structured conic cotangent without the rows any camera sees ill-conditioned."""
    cls = _classes(case) if len(case.poses) == 1 else _union_classes(case)
    if group == "conic_struct":
        ill = np.zeros(N, bool)
        for ci in range(len(case.poses)):
            ill |= _ill_conditioned(case, ci)
        cls = {k: v & ~ill for k, v in cls.items()}
    return cls


def _case_name(case):
    for table, prefix in ((SWEEP, "gsplat/"), (MODELS, "gsplat/"), (INRIA_VARIANTS, "inria/")):
        for k, v in table.items():
            if v == case:
                return prefix + k
    return {GSPLAT: "gsplat", INRIA: "inria", GSPLAT_C3: "gsplat/C3", NARROW: "gsplat/narrow"}[case]


def _asserted(case, groups=None):
    """Every (group, output, class) a GPU test of `case` holds to 1e-4."""
    for group in (groups or _groups(case)):
        for out in _outputs_of(case):
            for cls in _grad_classes(case, group):
                if (_case_name(case), group, out, cls) not in NOT_FP32:
                    yield group, out, cls


def _scaled_worst(got, ref):
    rms = float(np.sqrt(np.mean(ref * ref))) + 1e-30
    return float((np.abs(got - ref) / (np.abs(ref) + rms)).max()) if ref.size else 0.0


ALL_GRADIENT_CASES = [(GSPLAT, None), (GSPLAT_C3, None), (INRIA, None), (NARROW, ("comp",))] + [(c, (SWEEP_GROUP,)) for c in SWEEP.values()] \
    + [(c, None) for c in MODELS.values()] + [(c, INRIA_VARIANT_GROUPS) for c in INRIA_VARIANTS.values()]


# ---------------------------------------------------------------------------------------------
# no GPU: the scene and the calibration
# ---------------------------------------------------------------------------------------------
def test_scene_has_every_class():
    limx, limy = _limits()
    for case, visible, table in ((GSPLAT, 1963, (793, 235, 480, 455)), (INRIA, 1796, (792, 216, 444, 344))):
        r = _ref(case)
        pc, keep = r.pc[0], r.keep[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            cx, cy = np.abs(pc[:, 0] / pc[:, 2]) > limx, np.abs(pc[:, 1] / pc[:, 2]) > limy
        counts = tuple(int((keep & m).sum()) for m in (~cx & ~cy, cx & ~cy, ~cx & cy, cx & cy))
        cls = {k: int(v.sum()) for k, v in _classes(case).items()}
        well = {k: int(v.sum()) for k, v in _grad_classes(case, "conic_struct").items()}
        print(_case_name(case), "visible", int(keep.sum()), "none / x / y / both", counts, "classes", cls, "of them kappa <= 16", well)
        assert int(keep.sum()) == visible and counts == table      # the table of the module docstring
        assert cls.get("near_band", 100) >= 100 and min(v for k, v in well.items() if k != "near_band") >= MIN_CLASS_ROWS, (cls, well)
    z = _ref(GSPLAT).pc[0][:, 2]
    behind, sliver, band = int((z < 0).sum()), int(((z >= 0) & (z < 0.01)).sum()), (z >= 0.01) & (z < 0.2)
    print("behind", behind, "0<=z<0.01", sliver, "0.01<=z<0.2", int(band.sum()), "of them visible (gsplat)", int((band & _ref(GSPLAT).keep[0]).sum()))
    assert behind >= MIN_CLASS_ROWS and int(band.sum()) >= MIN_CLASS_ROWS and sliver > 0
    assert int((band & _ref(GSPLAT).keep[0]).sum()) >= 100 and not (band & _ref(INRIA).keep[0]).any()
    # the three poses of the batched case are all inside the cloud, and each clamps and culls
    for ci in range(3):
        c = _classes(GSPLAT_C3, ci)
        assert min(int(v.sum()) for k, v in c.items() if k != "near_band") >= MIN_CLASS_ROWS, {k: int(v.sum()) for k, v in c.items()}
        assert int((_ref(GSPLAT_C3).pc[ci][:, 2] < 0).sum()) >= MIN_CLASS_ROWS
    assert int(_classes(MODELS["fisheye"])["near_axis"].sum()) >= 24 and int(_classes(MODELS["fisheye"])["wide_angle"].sum()) >= MIN_CLASS_ROWS


def test_fp32_oracle_holds_half_the_bar():
    """The bar's calibration (module docstring).  For every case: no row sits on a plane or on a clamp limit; the fp32 oracle takes the
    fp64 oracle's decisions on all but at most 4 rows; and it holds 5e-5 on every combination the GPU tests assert.  fp32 sums differ
    from one host CPU to the next, so the list is kept a factor of two away from that bound on either side: where it was written every
    combination beyond 2.5e-5 was listed, and a listed combination must still be beyond 1e-5 wherever this runs (the list excuses nothing
    the fp32 oracle holds with room to spare)."""
    failures, stale = [], []
    for case, groups in ALL_GRADIENT_CASES:
        name = _case_name(case)
        r64, r32 = _ref(case), _ref(case, torch.float32)
        differ = np.zeros(N, bool)
        for ci in range(len(case.poses)):
            on_plane, on_limit = _threshold_rows(case, ci)
            assert not on_plane.any() and not on_limit.any(), (name, ci, int(on_plane.sum()), int(on_limit.sum()))
            differ |= r64.radii[ci] != r32.radii[ci]
        assert int(differ.sum()) <= MAX_LEFT_OUT, (name, int(differ.sum()))
        if case in (GSPLAT, INRIA):
            assert not differ.any()      # the scene as chosen: the same radii in fp32 and fp64 on every row
        worst = {}
        for group in (groups or _groups(case)):
            g64, g32 = r64.grads(group), r32.grads(group)
            for out in _outputs_of(case):
                for cls, rows in _grad_classes(case, group).items():
                    rows = rows & ~differ
                    w = _scaled_worst(g32[out][rows], g64[out][rows])
                    worst[(group, out)] = max(worst.get((group, out), 0.0), w)
                    listed = (name, group, out, cls) in NOT_FP32
                    if w > HALF_BAR and not listed:
                        failures.append(f"    ({name!r}, {group!r}, {out!r}, {cls!r}): {w:.1e},")
                    if w <= LISTED_FLOOR and listed:
                        stale.append((name, group, out, cls, w))
        print(f"    {name:<20}" + "  ".join(f"{g}/{o} {w:.1e}" for (g, o), w in worst.items()))
    assert not failures, "the fp32 oracle misses 5e-5 on combinations that are not listed in NOT_FP32:\n" + "\n".join(failures)
    assert not stale, f"NOT_FP32 lists combinations the fp32 oracle holds to {LISTED_FLOOR:g}: {stale}"
    # the least that must end up asserted: v_means for every group and class of both APIs, v_scales and v_quats under one conic group
    for case in (GSPLAT, INRIA):
        held = set(_asserted(case))
        for group in _groups(case):
            for cls in _grad_classes(case, group):
                # (v_compensations: not in this scene, see NOT_FP32; the narrow splats of NARROW hold it, below)
                assert group == "comp" or (group, "means", cls) in held, (case.api, group, cls)
        assert any(all((group, out, cls) in held for out in ("scales", "quats") for cls in _grad_classes(case, group))
                   for group in ("conic_rand", "conic_struct")), case.api
    assert {("comp", out, "inside") for out in ("means", "scales", "quats")} <= set(_asserted(NARROW, ("comp",)))


# ---------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib, ops
    _lib.lib()       # raises if the extension is missing: no silent fallback
    return ops


def _dev():
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _left_out(case, gpu_radii):
    """bool [C, N]: the rows on a threshold (module docstring) — at most 4 per case."""
    r = _ref(case)
    left = np.zeros((len(case.poses), N), bool)
    for ci in range(len(case.poses)):
        on_plane, on_limit = _threshold_rows(case, ci)
        left[ci] = on_plane | on_limit | (gpu_radii[ci] != r.radii[ci])
    n = int(left.any(axis=0).sum())
    print(f"{_case_name(case)}: {n} row(s) left out (radius differs from the fp64 oracle's, or on a plane / a clamp limit)")
    assert n <= MAX_LEFT_OUT, f"{_case_name(case)}: {n} rows on a threshold or with a radius other than the oracle's (at most {MAX_LEFT_OUT})"
    return left


def _check_forward(case, got, gpu_radii, left, classes_of=_classes):
    """Outputs per class at the tolerances of test_hip_parity.py::test_projection_vs_oracle_fp64_batched_cameras (and of the golden test
    for depths and compensations); culled rows exactly zero in every output."""
    r = _ref(case)
    for ci in range(len(case.poses)):
        culled = gpu_radii[ci] == 0
        for name, g in got.items():
            assert not g[ci][culled].any(), f"{_case_name(case)} camera {ci}: {name} of a culled row is not zero"
        for cls, rows in classes_of(case, ci).items():
            rows = rows & ~left[ci]
            tag = f"{_case_name(case)} cam{ci} {cls}"
            for name, g in got.items():
                ref = r.out(name)[ci][rows]
                if name == "conic":
                    assert_close_scaled(g[ci][rows], ref, 2e-4, f"{tag} conics", 0.999, rel_all=5e-2)
                else:
                    rtol, atol = {"xy": (1e-5, 2e-3), "depth": (1e-5, 1e-6), "comp": (2e-4, 1e-6), "color": (2e-5, 3e-6)}[name]
                    np.testing.assert_allclose(g[ci][rows], ref, rtol=rtol, atol=atol, err_msg=f"{tag} {name}")


def _check_grads(case, grads_of, gpu_radii, left, groups=None):
    """grads_of(group) -> {leaf: gradient}; every (group, leaf, class) the fp32 oracle holds to 5e-5 is held to 1e-4 here; a row no
    camera kept has an exactly zero gradient."""
    r = _ref(case)
    name = _case_name(case)
    dead, skip = (gpu_radii == 0).all(axis=0), left.any(axis=0)
    for group in (groups or _groups(case)):
        got, ref = grads_of(group), r.grads(group)
        for out in _outputs_of(case):
            g = _np(got[out])
            assert g.shape == ref[out].shape, (out, g.shape, ref[out].shape)
            assert not g[dead].any(), f"{name} {group}: v_{out} of a culled row is not zero"
            for cls, rows in _grad_classes(case, group).items():
                rows = rows & ~skip
                listed = (name, group, out, cls) in NOT_FP32
                print(f"{name:<20} {group:<13} v_{out:<7} {cls:<10} {int(rows.sum()):5d} rows  worst {_scaled_worst(g[rows], ref[out][rows]):.2e}"
                      + ("   (not asserted: NOT_FP32)" if listed else ""))
                if not listed:
                    assert_close_scaled(g[rows], ref[out][rows], REL, f"{name} {group} v_{out} [{cls}]", frac_ok=1.0)


# ---- gsplat -------------------------------------------------------------------------------------
def _gsplat_cams(case):
    cams = [_camera(p) for p in case.poses]
    vms = torch.stack([c["world_to_camera"].T for c in cams]).float().contiguous().to(_dev())
    Ks = torch.stack([torch.tensor([[FX, 0, c["cx"]], [0, FY, c["cy"]], [0, 0, 1.0]]) for c in cams]).float().to(_dev())
    return cams, vms, Ks


def _gsplat_gpu(hip, case, v0=False):
    """(leaves, outputs [C, N, ...], radii [C, N] numpy, tiles_hit or None) through `project_gaussians` (v0) or `fully_fused_projection`."""
    p = _params(case)
    leaves = {k: p[k].to(_dev()).requires_grad_(True) for k in ("means", "scales", "quats")}
    cams, vms, Ks = _gsplat_cams(case)
    m, s, q = leaves["means"], leaves["scales"], leaves["quats"]
    if v0:
        assert len(case.poses) == 1 and case.model == "pinhole" and not case.clip and case.far >= 1e9
        xy, depth, radii, conic, comp, tiles, _ = hip.project_gaussians(m, s, case.smod, q, vms[0], FX, FY, cams[0]["cx"], cams[0]["cy"], H, W, 16,
                                                                      clip_thresh=case.near, filter_2d_kernel_size=case.eps2d)
        outs = {"xy": xy[None], "depth": depth[None], "conic": conic[None], "comp": comp[None]}
        return leaves, outs, radii[None].cpu().numpy(), tiles[None].cpu().numpy()
    clip = _ref(case).clip if case.clip else 0.0
    radii, xy, depth, conic, comp = hip.fully_fused_projection(
        m, None, q, s, vms, Ks, W, H, eps2d=case.eps2d, near_plane=case.near, far_plane=case.far, radius_clip=clip,
        calc_compensations=True, camera_model=case.model, scale_modifier=case.smod)
    return leaves, {"xy": xy, "depth": depth, "conic": conic, "comp": comp}, radii.cpu().numpy(), None


def _autograd_grads(case, leaves, outs):
    def grads_of(group):
        cots = _cotangents(case)[group]
        g = torch.autograd.grad([outs[k] for k in cots], list(leaves.values()), [v.float().to(_dev()) for v in cots.values()], retain_graph=True)
        return dict(zip(leaves, g))
    return grads_of


def _run_gsplat(hip, case, v0=False, groups=None, classes_of=_classes):
    leaves, outs, radii, tiles = _gsplat_gpu(hip, case, v0)
    left = _left_out(case, radii)
    if tiles is not None:
        ok = ~left[0]
        assert np.array_equal(tiles[0][ok], _ref(case).tiles[0][ok]), "tiles_hit differs from the oracle's"
    _check_forward(case, {k: _np(v) for k, v in outs.items()}, radii, left, classes_of)
    _check_grads(case, _autograd_grads(case, leaves, outs), radii, left, groups)
    return radii


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["project_gaussians", "fully_fused_projection"])
def test_gsplat_projection_inside_the_cloud(hip, entry):
    """C = 1: forward per class, radii and tiles_hit exact, culled rows zero, then every cotangent group per class.  The clamped classes
    pin the gsplat rule: the exact derivative of clamp(x / z) z (`ewa_bwd<true>`)."""
    radii = _run_gsplat(hip, GSPLAT, v0=(entry == "project_gaussians"))
    z = _ref(GSPLAT).pc[0][:, 2]
    assert not radii[0][z < 0.0099].any() and int((radii[0][(z >= 0.0101) & (z < 0.2)] > 0).sum()) >= 100


@pytest.mark.gpu
def test_gsplat_compensation_gradient_on_narrow_splats(hip):
    """The `v_compensations` group where fp32 can hold it: the same cloud and camera with the scales x 0.25, splats about a pixel wide,
    compensations 0.2 ... 0.75 (600 visible rows, none of them clamped: a splat this small is on a tile only when it is on the screen)."""
    comp = _ref(NARROW).out("comp")[0][_ref(NARROW).keep[0]]
    assert int(_ref(NARROW).keep[0].sum()) >= MIN_CLASS_ROWS and 0.3 < float(np.median(comp)) < 0.7
    _run_gsplat(hip, NARROW, groups=("comp",))


@pytest.mark.gpu
def test_gsplat_projection_three_cameras_inside_the_cloud(hip):
    """C = 3 poses inside the cloud: the atomic path (`project_bwd_kernel<true>`), gradients summed over the cameras against the oracle's
    sum; the op hands the kernel pre-zeroed v_* rows, as the header requires."""
    _run_gsplat(hip, GSPLAT_C3)


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(SWEEP))
def test_gsplat_projection_argument_sweep(hip, which):
    """near_plane (against the oracle's min_depth), far_plane, radius_clip (`radius <= clip` culls; in "clip_equal" the clip EQUALS the
    radius of a dozen splats), eps2d, scale_modifier / glob_scale: forward, mask, and the structured conic gradient group."""
    case, r = SWEEP[which], _ref(SWEEP[which])
    base = _ref(GSPLAT).keep[0]
    if case.clip:
        frac = 1.0 - r.keep[0].sum() / base.sum()
        on_clip = int((_ref(GSPLAT).radii[0][base] == r.clip).sum())
        print(f"{which}: clip {r.clip}, culls {frac:.2f} of the visible rows, {on_clip} radii equal to it")
        # more rows ON the clip than the left-out allowance could excuse: `radius < clip` cannot hide among the rows on a threshold
        assert 0.25 <= frac <= 0.75 and (on_clip > MAX_LEFT_OUT if case.clip == "equal" else on_clip == 0)
    if which in ("near0.2", "near0.5", "far1.2"):
        assert int((base & ~r.keep[0]).sum()) >= 100 and int(r.keep[0].sum()) >= MIN_CLASS_ROWS      # the plane cuts through the cloud (near 0.2: the 108 rows of the band)
    v0 = which in ("smod0.5", "smod2", "eps0.1", "near0.2")      # the v0 entry's glob_scale, filter_2d_kernel_size, clip_thresh
    radii = _run_gsplat(hip, case, v0=v0, groups=(SWEEP_GROUP,))
    assert int(((radii[0] > 0) != r.keep[0]).sum()) <= MAX_LEFT_OUT
    if case.clip == "equal":      # the rule is `radius <= clip`: a radius equal to the clip is culled
        assert not radii[0][_ref(GSPLAT).radii[0] == r.clip].any()


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(MODELS))
def test_gsplat_projection_other_camera_models_inside_the_cloud(hip, model):
    """"ortho" and "fisheye" on the same scene against `O.camera_jacobian`; fisheye classes: next to the axis (r < 1e-3 z, planted), wide
    angle (theta > 60 degrees), between."""
    _run_gsplat(hip, MODELS[model])


@pytest.mark.gpu
def test_gsplat_backward_reads_strided_cotangents(hip):
    """C == 1 through the C ABI: `v_means2d_stride` / `v_conics_stride` read columns of one packed row buffer (as compositing's backward
    leaves them); the results are bit-equal to dense inputs, and equal to the op's."""
    from gspl_amd import _lib as L
    case = GSPLAT
    leaves, outs, radii, _ = _gsplat_gpu(hip, case)
    cots = _cotangents(case)
    v_xy, v_con = [cots[g][k][0].float().to(_dev()).contiguous() for g, k in (("xy", "xy"), ("conic_struct", "conic"))]
    v_dep, v_cmp = [cots[g][g][0].float().to(_dev()).contiguous() for g in ("depth", "comp")]
    _, vms, Ks = _gsplat_cams(case)
    rad = torch.from_numpy(radii[0]).to(_dev())
    m, s, q = [leaves[k].detach() for k in ("means", "scales", "quats")]
    RS = 16
    packed = torch.randn(N, RS, device=_dev())
    packed[:, 0:2], packed[:, 2:5] = v_xy, v_con

    def bwd(xy, s2, con, s3):
        out = [torch.full((N, k), 7.0, device=_dev()) for k in (3, 3, 4)]      # C == 1: overwritten, not accumulated
        L.call("gspl_project_bwd", 1, N, L.ptr(m), L.ptr(s), L.ptr(q), L.ptr(vms), L.ptr(Ks), W, H, case.smod, case.eps2d, L.CAMERA_MODELS[case.model],
               L.ptr(rad), xy, s2, L.ptr(v_dep), con, s3, L.ptr(v_cmp), L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.stream())
        return out
    dense = bwd(L.ptr(v_xy), 0, L.ptr(v_con), 0)
    strided = bwd(L.ptr(packed), RS, L.ptr(packed, offset_bytes=8), RS)
    op = torch.autograd.grad([outs["xy"], outs["depth"], outs["conic"], outs["comp"]], list(leaves.values()),
                             [v_xy[None], v_dep[None], v_con[None], v_cmp[None]])
    for a, b, c, name in zip(dense, strided, op, ("v_means", "v_scales", "v_quats")):
        assert torch.equal(a, b), f"{name}: strided cotangents give other bits than dense ones"
        assert torch.equal(a, c), f"{name}: the C ABI gives other bits than the op"
        assert bool((a[rad > 0] != 0).any()) and not bool(a[rad == 0].any())


# ---- Inria --------------------------------------------------------------------------------------
def _inria_inputs(case):
    p = {k: v.to(_dev()).contiguous() for k, v in _params(case).items()}
    cam = _camera(case.poses[0])
    for k in ("world_to_camera", "full_projection", "camera_center"):
        p[k] = cam[k].float().contiguous().to(_dev())
    return p, cam


def _inria_fwd(case, phases=None):
    """`gspl_inria_preprocess_fwd` (argument order: include/gspl_hip.h, ops/inria.py); outputs pre-filled with a value no row has."""
    from gspl_amd import _lib as L
    p, cam = _inria_inputs(case)
    f = lambda *shape, dtype=torch.float32: torch.full(shape, 7, dtype=dtype, device=_dev())
    o = dict(radii=f(N, dtype=torch.int32), xy=f(N, 2), depth=f(N), conic=f(N, 3), color=f(N, 3), clamped=f(N, 3, dtype=torch.uint8), cov3d=f(N, 6))
    for ph in (phases or (L.GSPL_INRIA_ALL,)):
        L.call("gspl_inria_preprocess_fwd", N, 3, 16, L.ptr(p["means"]), L.ptr(p.get("scales")), L.ptr(p.get("quats")), L.ptr(p.get("cov6")),
               L.ptr(p.get("shs")), None, L.ptr(p.get("colors")), L.ptr(p["world_to_camera"]), L.ptr(p["full_projection"]), L.ptr(p["camera_center"]),
               W, H, 16, float(cam["tanfovx"]), float(cam["tanfovy"]), case.smod,
               L.ptr(o["radii"]), L.ptr(o["xy"]), L.ptr(o["depth"]), L.ptr(o["conic"]), L.ptr(o["color"]), L.ptr(o["clamped"]), L.ptr(o["cov3d"]),
               None, ph, L.stream())
    return p, cam, o


def _inria_bwd(case, p, cam, o, v_xy, v_con, v_col, packed_stride=0):
    """`gspl_inria_preprocess_bwd` with the three cotangents handed over directly: dense, or as columns of one packed [N, stride] buffer
    (x y | a b c | opacity | r g b, as compositing's backward leaves them)."""
    from gspl_amd import _lib as L
    f = lambda *shape: torch.full(shape, 7.0, device=_dev())
    v = dict(means=f(N, 3), ndc=f(N, 3))
    if case.cov_pre:
        v["cov6"] = f(N, 6)
    else:
        v["scales"], v["quats"] = f(N, 3), f(N, 4)
    v["colors" if case.colors_pre else "shs"] = f(N, 3) if case.colors_pre else f(N, 16, 3)
    if packed_stride:
        packed = torch.randn(N, packed_stride, device=_dev())
        packed[:, 0:2], packed[:, 2:5], packed[:, 6:9] = v_xy, v_con, v_col
        a_xy, a_con, a_col = L.ptr(packed), L.ptr(packed, offset_bytes=8), L.ptr(packed, offset_bytes=24)
    else:
        a_xy, a_con, a_col = L.ptr(v_xy), L.ptr(v_con), L.ptr(v_col)
    L.call("gspl_inria_preprocess_bwd", N, 3, 16, L.ptr(p["means"]), L.ptr(p.get("scales")), L.ptr(p.get("quats")), L.ptr(o["cov3d"]),
           L.ptr(p.get("shs")), None, L.ptr(p["world_to_camera"]), L.ptr(p["full_projection"]), L.ptr(p["camera_center"]),
           W, H, float(cam["tanfovx"]), float(cam["tanfovy"]), case.smod, L.ptr(o["radii"]), L.ptr(o["clamped"]),
           a_xy, a_con, a_col, packed_stride,
           L.ptr(v["means"]), L.ptr(v.get("scales")), L.ptr(v.get("quats")), L.ptr(v.get("cov6")), L.ptr(v.get("shs")), None, L.ptr(v.get("colors")),
           L.ptr(v["ndc"]), None, None, None, L.stream())
    return v


def _inria_cots(case, group):
    """(v_means2d, v_conics, v_colors) of one group: the other two are zero."""
    cots = _cotangents(case)[group]
    z = lambda k: torch.zeros(N, k, device=_dev())
    pick = lambda name, k: cots[name][0].float().to(_dev()).contiguous() if name in cots else z(k)
    return pick("xy", 2), pick("conic", 3), pick("color", 3)


def _run_inria(case, groups=None):
    p, cam, o = _inria_fwd(case)
    radii = o["radii"].cpu().numpy()[None]
    left = _left_out(case, radii)
    r = _ref(case)
    _check_forward(case, {k: _np(o[k])[None] for k in ("xy", "depth", "conic", "color")}, radii, left)
    # the 0.2 near plane culls the whole 0.01 ... 0.2 band that gsplat's 0.01 keeps; means2d is integer-centred: ((ndc + 1) W - 1) / 2
    z = r.pc[0][:, 2]
    assert not radii[0][z <= 0.2 * (1 - 1e-5)].any() and int((z[radii[0] > 0] < 0.25).sum()) > 0
    vis = (radii[0] > 0) & ~left[0]
    if not case.colors_pre:
        lv = {k: v.double() for k, v in _params(case).items()}
        raw = _np(O.eval_sh(3, lv["shs"], lv["means"] - cam["camera_center"].double())) + 0.5
        firm = vis[:, None] & (np.abs(raw) > 1e-5)
        assert np.array_equal(o["clamped"].cpu().numpy().astype(bool)[firm], (raw < 0)[firm]) and int((raw < 0)[firm].sum()) >= 40      # (48 ... 102 colour channels are clamped)
    if case.cov_pre:
        assert torch.equal(o["cov3d"], p["cov6"])

    ndc = {}

    def grads_of(group):
        v_xy, v_con, v_col = _inria_cots(case, group)
        v = _inria_bwd(case, p, cam, o, v_xy, v_con, v_col)
        ndc[group] = (v.pop("ndc"), v_xy)
        return v
    _check_grads(case, grads_of, radii, left, groups)
    # v_means2d_ndc = the pixel gradient x 0.5 (W, H), third column zero, culled rows zero
    for group, (got, v_xy) in ndc.items():
        want = torch.zeros(N, 3, device=_dev())
        want[:, 0], want[:, 1] = v_xy[:, 0] * 0.5 * W, v_xy[:, 1] * 0.5 * H      # (0.5 W and 0.5 H are powers of two times small integers: exact)
        want[o["radii"] <= 0] = 0
        assert torch.equal(got, want), f"{_case_name(case)} {group}: v_means2d_ndc"
    return p, cam, o


@pytest.mark.gpu
def test_inria_preprocess_inside_the_cloud():
    """Forward against `O.inria_preprocess` + `O.sh_colors`; backward with direct v_means2d / v_conics / v_colors, one group at a time:
    v_means, v_scales, v_quats, v_shs per class.  The clamped classes pin the Inria rule: a clamped coordinate contributes no gradient
    (`ewa_bwd<false>`)."""
    _run_inria(INRIA)


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(INRIA_VARIANTS))
def test_inria_preprocess_variants(which):
    """scale_modifier 0.5 / 2, `cov3D_precomp` (with `v_cov3d_precomp`), `colors_precomp` (with `v_colors_precomp`)."""
    _run_inria(INRIA_VARIANTS[which], groups=INRIA_VARIANT_GROUPS)


@pytest.mark.gpu
def test_inria_phases_and_packed_cotangents_are_bit_equal():
    """GEOMETRY then COLOURS gives the bits of ALL; cotangents read as columns of one packed row buffer (`grad_stride`) give the bits of
    dense ones."""
    from gspl_amd import _lib as L
    p, cam, whole = _inria_fwd(INRIA)
    _, _, split = _inria_fwd(INRIA, phases=(L.GSPL_INRIA_GEOMETRY, L.GSPL_INRIA_COLOURS))
    for k in whole:
        assert torch.equal(whole[k], split[k]), f"{k}: GEOMETRY then COLOURS differs from ALL"
    v_xy, v_con, v_col = _inria_cots(INRIA, "xy")[0], _inria_cots(INRIA, "conic_struct")[1], _inria_cots(INRIA, "color")[2]
    dense = _inria_bwd(INRIA, p, cam, whole, v_xy, v_con, v_col)
    for stride in (9, 16):
        packed = _inria_bwd(INRIA, p, cam, whole, v_xy, v_con, v_col, packed_stride=stride)
        for k in dense:
            assert torch.equal(dense[k], packed[k]), f"v_{k}: packed cotangents (stride {stride}) give other bits than dense ones"
    vis = whole["radii"] > 0
    assert all(bool((dense[k][vis] != 0).any()) for k in dense)

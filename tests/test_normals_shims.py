"""The depth-to-normal route without a GPU: the fp64 oracle of tests/normals_oracle.py against the plugin's existing torch classmethod
(and the reference's, where its tree is importable), the `gsplat.utils` stand-in of `gspl_amd.compat`, the reference's unedited
`internal.metrics.normal_reg` and `GS2DMetrics` next to `gspl_amd.surface.HipGS2DMetrics` (tests/normals_reference_worker.py, in a
process of its own), and the contract of the new ops: GPU only, and not called by the default plugin."""
import json
import os
import subprocess
import sys

import pytest
import torch

from oracle import gsplat_oracle as O
import normals_oracle as NO

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = os.environ.get("GSPL_REFERENCE_ROOT", "/root/reference")
needs_reference = pytest.mark.skipif(not os.path.exists(os.path.join(REF_ROOT, "internal", "renderers", "vanilla_2dgs_renderer.py")),
                                     reason="reference tree not present")


def _camera(W=50, H=37):
    from test_package_shims import _Cam
    return _Cam(O.synthetic_camera(W, H, 70.0, 68.0))


def _plugin_inputs(W=50, H=37, seed=2):
    from gspl_amd.renderers import HipVanilla2DGSRenderer
    cam = _camera(W, H)
    depth = NO.case_depth(H, W, seed).double()
    normal_rot, rays = HipVanilla2DGSRenderer.camera_matrices(cam, depth)
    return cam, depth, normal_rot, rays


def test_oracle_equals_the_plugins_classmethod():
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipVanilla2DGSRenderer
    cam, depth, normal_rot, rays = _plugin_inputs()
    assert rays.dtype == torch.float64 and torch.equal(normal_rot, cam.world_to_camera[:3, :3])
    ref = HipVanilla2DGSRenderer.depth_to_normal(cam, depth[None])
    got = NO.depth_to_normal(depth, rays)
    assert got.shape == ref.shape == (37, 50, 3)
    assert float((got - ref).abs().max()) <= 1e-12
    assert float(got[1:-1, 1:-1].norm(dim=-1).min()) > 0.999 and float(got[0].abs().max()) == 0.0 and float(got[:, -1].abs().max()) == 0.0
    assert torch.equal(NO.depth_to_normal(depth, rays, channels_first=True), got.permute(2, 0, 1))
    for shape in ((1, 1), (2, 5), (5, 2)):
        assert float(NO.depth_to_normal(torch.ones(shape, dtype=torch.float64), rays).abs().max()) == 0.0


def test_camera_matrices_are_kept_on_the_camera_and_follow_edits():
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipVanilla2DGSRenderer
    cam, depth, normal_rot, rays = _plugin_inputs()
    again = HipVanilla2DGSRenderer.camera_matrices(cam, depth)
    assert again[0] is normal_rot and again[1] is rays
    other = HipVanilla2DGSRenderer.camera_matrices(cam, depth.float())
    assert other[1].dtype == torch.float32 and other[1] is not rays
    cam.world_to_camera.mul_(1.0)                            # modified in place: the version counter moves
    assert HipVanilla2DGSRenderer.camera_matrices(cam, depth.float())[1] is not other[1]


@needs_reference
def test_oracle_equals_the_references_classmethod(monkeypatch):
    import gspl_amd  # noqa: F401
    from gspl_amd import compat
    from gspl_amd.renderers import HipVanilla2DGSRenderer
    compat.install()
    from test_package_shims import _stubs
    _stubs()
    import internal.renderers.vanilla_2dgs_renderer as vr
    # the reference builds its pixel grid with device='cuda'; on the CPU the plugin's device-agnostic restatement of that one static
    # method stands in for it (as in tests/test_surfel_shims.py); the stencil under test is the reference's own
    monkeypatch.setattr(vr.Vanilla2DGSRenderer, "depths_to_points", staticmethod(HipVanilla2DGSRenderer.depths_to_points))
    cam, depth, _, rays = _plugin_inputs(seed=5)
    ref = vr.Vanilla2DGSRenderer.depth_to_normal(cam, depth[None])
    assert float((NO.depth_to_normal(depth, rays) - ref).abs().max()) <= 1e-12


def _gsplat_stand_in():
    import gspl_amd  # noqa: F401
    from gspl_amd import compat
    compat.install()
    import gsplat
    if "gspl_amd" not in (gsplat.__doc__ or ""):
        pytest.skip("a real gsplat package is installed")


def test_gsplat_utils_stand_in_resolves_and_has_the_published_semantics(monkeypatch):
    _gsplat_stand_in()
    from gsplat.utils import depth_to_normal
    from gspl_amd import ops
    monkeypatch.setattr(ops, "depth_to_normal", NO.depth_to_normal)
    H, W = 9, 11
    g = torch.Generator().manual_seed(1)
    depths = 2 + torch.rand(2, 3, H, W, 1, generator=g, dtype=torch.float64)
    c2w = torch.eye(4, dtype=torch.float64).repeat(2, 3, 1, 1)
    c2w[..., :3, :3] = NO.case_rotation(4)
    c2w[..., :3, 3] = torch.randn(2, 3, 3, generator=g, dtype=torch.float64)
    K = torch.tensor([[20.0, 0, 5.2], [0, 21.0, 4.4], [0, 0, 1]], dtype=torch.float64).repeat(2, 3, 1, 1)
    for z_depth in (True, False):
        out = depth_to_normal(depths, c2w, K, z_depth=z_depth)
        assert out.shape == (2, 3, H, W, 3)
        # the published formulation, written out: directions through pixel centres at +0.5, optional normalisation, the stencil
        x, y = torch.meshgrid(torch.arange(W, dtype=torch.float64), torch.arange(H, dtype=torch.float64), indexing="xy")
        dirs = torch.stack([(x - 5.2 + 0.5) / 20.0, (y - 4.4 + 0.5) / 21.0, torch.ones_like(x)], dim=-1) @ NO.case_rotation(4).T
        if not z_depth:
            dirs = torch.nn.functional.normalize(dirs, dim=-1)
        for i in range(2):
            for j in range(3):
                pts = c2w[i, j, :3, 3] + depths[i, j] * dirs
                dx = pts[2:, 1:-1] - pts[:-2, 1:-1]
                dy = pts[1:-1, 2:] - pts[1:-1, :-2]
                n = torch.nn.functional.pad(torch.nn.functional.normalize(torch.cross(dx, dy, dim=-1), dim=-1), (0, 0, 1, 1, 1, 1))
                assert float((out[i, j] - n).abs().max()) <= 1e-12
    single = depth_to_normal(depths[0, 0], c2w[0, 0], K[0, 0])
    assert single.shape == (H, W, 3) and torch.equal(single, depth_to_normal(depths, c2w, K)[0, 0])
    assert float((NO.gsplat_depth_to_normal(depths[0, 0], c2w[0, 0], K[0, 0]) - single).abs().max()) <= 1e-12
    with pytest.raises(ImportError):
        from gsplat.utils import rasterize_to_vis_aware_weights  # noqa: F401  (still not built)


@needs_reference
def test_reference_normal_reg_and_gs2d_metrics_run_on_the_stand_ins():
    r = subprocess.run([sys.executable, os.path.join(HERE, "normals_reference_worker.py"), REF_ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    if not d["stand_in"]:
        pytest.skip("a real gsplat package is installed")
    assert d["normal_reg_uses_the_stand_in"]
    assert d["normal_reg_loss"] == pytest.approx(d["normal_reg_expected"], rel=1e-12) and 0.01 < d["normal_reg_loss"] < 1.0
    assert d["normal_reg_entries"] == ["flatten_loss", "loss", "normal_loss", "flatten_loss", "normal_loss"]
    assert d["depth_to_normal_calls"] == [[[37, 50], False]]
    assert d["subclass"] and d["fields"] == [0.05, 100.0, 0.05, 0.0]
    for ref, ours in d["gs2d"]:
        assert ours[3] == ref[3] == ["dist_loss", "normal_loss"]
        assert ours[:3] == pytest.approx(ref[:3], rel=1e-12, abs=1e-15)
    assert d["gs2d"][0][1][1:3] == [0.0, 0.0] and d["gs2d"][1][1][1] == 0.0 and d["gs2d"][1][1][2] > 0 and d["gs2d"][2][1][1] > 0


def test_stand_alone_metric_placeholder_says_what_it_needs():
    import gspl_amd  # noqa: F401
    from gspl_amd import surface
    if surface._GS2DMetrics is not None:
        pytest.skip("the reference tree is importable in this process")
    cfg = surface.HipGS2DMetrics()
    assert (cfg.lambda_normal, cfg.lambda_dist) == (0.05, 0.0)
    with pytest.raises(RuntimeError, match="reference"):
        cfg.instantiate()


def test_cpu_tensors_are_refused():
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    A = torch.eye(3)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.depth_to_normal(torch.ones(5, 6), A)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.surfel_maps(torch.ones(7, 5, 6), A, A, 0.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.surface_reg(torch.ones(3, 5, 6), torch.ones(3, 5, 6), torch.ones(5, 6))
    from gsplat.utils import depth_to_normal as stand_in
    import gsplat
    if "gspl_amd" in (gsplat.__doc__ or ""):
        with pytest.raises(RuntimeError, match="GPU only"):
            stand_in(torch.ones(5, 6, 1), torch.eye(4), torch.eye(3))


def test_default_plugin_never_calls_surfel_maps(monkeypatch):
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    from gspl_amd.renderers import HipVanilla2DGSRenderer
    import gspl_amd.ops.surfel as surfel
    import surfel_oracle as SO
    from test_surfel_shims import _Model, _oracle_op, _scene
    calls, maps_calls = [], []
    monkeypatch.setattr(surfel, "rasterize_surfels", _oracle_op(calls))

    def oracle_maps(allmap, normal_rot, rays, depth_ratio):
        maps_calls.append(depth_ratio)
        return NO.surfel_maps(allmap, normal_rot, rays, depth_ratio)
    monkeypatch.setattr(ops, "surfel_maps", oracle_maps)
    params, cam, bg = _scene(n=200, W=40, H=32)
    from test_package_shims import _Cam
    assert HipVanilla2DGSRenderer().fused_maps is False
    plain = HipVanilla2DGSRenderer(depth_ratio=0.3)(_Cam(cam), _Model(params), bg)
    assert len(calls) == 1 and maps_calls == []
    fused = HipVanilla2DGSRenderer(depth_ratio=0.3, fused_maps=True)(_Cam(cam), _Model(params), bg)
    assert maps_calls == [0.3] and set(fused) == set(plain)
    for k in ("rend_alpha", "rend_normal", "view_normal", "rend_dist", "surf_depth", "surf_normal"):
        assert fused[k].shape == plain[k].shape, k
        assert float((fused[k] - plain[k]).abs().max()) <= 1e-9, k

"""Wide-feature compositing, the parts that need no GPU: the declared ABI, the plugin classes' surface, the CPU refusal and the
channel-slicing fp64 helper."""
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import feature_oracle as FO
from oracle import gsplat_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_points():
    from gspl_amd import _lib as L
    text = open(L.HEADER_PATH).read()
    for name in ("gspl_feature_fwd", "gspl_feature_bwd"):
        assert f"int {name}(" in text
        assert name in L.exported_symbols()
    assert L.ABI_VERSION == 39
    fwd, bwd = L._FUNCTIONS["gspl_feature_fwd"][2], L._FUNCTIONS["gspl_feature_bwd"][2]
    assert fwd[:5] == bwd[:5] == ("N", "n_isects", "D", "mode", "layout")
    assert "features" in fwd and "backgrounds" in fwd and "features" not in bwd and "backgrounds" not in bwd
    assert bwd[-3:] == ("v_out", "v_features", "stream") and fwd[-5:] == ("out", "out_alphas", "final_Ts", "last_ids", "stream")


def test_plugins_are_exported_and_load_without_optional_packages():
    # a fresh interpreter in which viser / clip / sklearn cannot be imported at all
    code = ("import sys\n"
            "for m in ('viser', 'clip', 'sklearn'): sys.modules[m] = None\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "import gspl_amd.renderers as R\n"
            "a = R.HipFeature3DGSRenderer(speedup=True, n_feature_dims=64)\n"
            "b = R.HipGSplatContrastiveFeatureRenderer()\n"
            "assert a.rasterize_batch == 32 and b.feature_map_width == -1\n"
            "assert set(a.get_available_outputs()) == {'rgb', 'features', 'features_vanilla_pca_2d', 'features_pca_3d', 'edited'}\n"
            "print('ok')\n")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stdout + res.stderr


def test_constructor_signatures_match_the_reference():
    from gspl_amd import renderers as R
    names = json.load(open(os.path.join(ROOT, "tests", "golden", "feature_renderer_signatures.json")))
    for cls, ref in ((R.HipFeature3DGSRenderer, "Feature3DGSRenderer"), (R.HipGSplatContrastiveFeatureRenderer, "GSplatContrastiveFeatureRenderer")):
        assert list(inspect.signature(cls.__init__).parameters) == names[ref]
    sig = inspect.signature(R.HipFeature3DGSRenderer.__init__).parameters
    assert (sig["feature_lr"].default, sig["feature_decoder_lr"].default, sig["rasterize_batch"].default) == (0.001, 0.0001, 32)
    assert inspect.signature(R.HipGSplatContrastiveFeatureRenderer.__init__).parameters["feature_map_width"].default == -1
    assert "ignored" in R.HipFeature3DGSRenderer.__init__.__doc__
    fwd = inspect.signature(R.HipGSplatContrastiveFeatureRenderer.forward).parameters
    assert list(fwd)[:6] == ["self", "viewpoint_camera", "pc", "bg_color", "scaling_modifier", "semantic_features"]
    assert list(inspect.signature(R.HipGSplatContrastiveFeatureRenderer.depth_forward).parameters) == ["self", "viewpoint_camera", "pc"]


def test_op_signature_and_cpu_tensors_raise():
    from gspl_amd import ops
    params = list(inspect.signature(ops.rasterize_features).parameters)
    like = [p for p in inspect.signature(ops.rasterize_gaussians).parameters if p != "absgrad"]
    assert params == [("features" if p == "colors" else p) for p in like]
    n = 5
    args = (torch.zeros(n, 2), torch.ones(n), torch.ones(n, dtype=torch.int32), torch.ones(n, 3), torch.ones(n, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.rasterize_features(*args, torch.zeros(n, 40), torch.ones(n, 1), 16, 16, 16)
    with pytest.raises(ValueError):
        ops.rasterize_features(*args, torch.zeros(n + 1, 40), torch.ones(n, 1), 16, 16, 16)
    with pytest.raises(NotImplementedError):
        ops.rasterize_features(*args, torch.zeros(n, 40), torch.ones(n, 1), 16, 16, 12)


def test_oracle_slicing_agrees_with_one_call():
    """12 channels in slices of 5 against ONE 12-channel oracle call: the forward exactly, the feature gradient to fp64 rounding (the
    oracle's backward adds the pixels' contributions from several threads, in no fixed order)."""
    W, H, n, D = 50, 34, 400, 12
    means, scales, quats, opac, _ = O.synthetic_scene(n, seed=3)
    cam = O.synthetic_camera(W, H, 260.0)
    res = O.project_gaussians(means, scales * 3.0, 1.0, quats, cam["world_to_camera"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], H, W)
    xys, depths, radii, conics, comp = res[0], res[1], res[2], res[3], res[4]
    g = torch.Generator().manual_seed(1)
    feats, bg = torch.rand(n, D, generator=g), torch.rand(D, generator=g)
    op = (opac.reshape(-1) * comp).float()
    _, _, flat, offs = O.isect_tiles(O.MODE_GSPLAT, xys, radii, depths, W, H)
    one = O.composite_fwd(O.MODE_GSPLAT, xys, conics, feats, op, bg, W, H, offs, flat)
    cut = FO.feature_fwd(O.MODE_GSPLAT, xys, conics, feats, op, bg, W, H, offs, flat, width=5)
    assert all(np.array_equal(a, b) for a, b in zip(one, cut))
    assert one[0].shape == (H, W, D) and float(one[1].max()) > 0.1
    v_out = torch.randn(H, W, D, generator=g).double().numpy()
    ref = O.composite_bwd(O.MODE_GSPLAT, xys, conics, feats, op, bg, W, H, offs, flat, one[1], one[2], v_out, None, fragile_px=one[3])
    got = FO.feature_bwd(O.MODE_GSPLAT, xys, conics, feats, op, bg, W, H, offs, flat, one[1], one[2], v_out, fragile_px=one[3], width=5)
    assert float(np.abs(got).max()) > 0
    np.testing.assert_allclose(got, ref["v_colors"], rtol=1e-12, atol=1e-13 * float(np.abs(got).max()))

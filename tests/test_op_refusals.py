"""The refusals of the route ops that need no device, pinned: every case names a bad call, the exception class and the substrings
its message must contain (the op where the message names one, the argument, and the fragment other tests and callers match).
tests/golden/op_refusals.json holds the class and the full text each case gave before the checks moved into `ops/_args.py`; the set of
cases there must equal the set here, so that none is dropped silently.  `python tests/test_op_refusals.py` records that file anew."""
import json
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "op_refusals.json")
f32, f64, i64 = torch.float32, torch.float64, torch.int64
Z = torch.zeros


def _ops():
    from gspl_amd import ops
    return ops


def _glossy(**bad):
    a = dict(degree=1, means=Z(4, 3), camera_center=Z(3), opacity_dc=Z(4, 1, 1), opacity_rest=Z(4, 3, 1))
    a.update(bad)
    return lambda: _ops().sh_view_opacities(*a.values())


def _select(**bad):
    P, L = 4, 3
    kw = {k: bad.pop(k) for k in list(bad) if k in ("visibility_filter", "boxes3d", "world_to_camera", "Ks")}
    a = dict(seg_start=Z(L * P + 1, dtype=i64), camera_center=Z(3), transform=torch.eye(3), box_min=Z(P, 2), box_max=torch.ones(P, 2),
             thresholds=torch.ones(L - 1), prev_lod=Z(P, dtype=torch.int8), prev_visible=torch.ones(P, dtype=torch.uint8))
    a.update(bad)
    return lambda: _ops().lod_select(*a.values(), **kw)


def _gather(out=None, **bad):
    R, K, P, L = 8, 4, 2, 2
    a = dict(seg_start=Z(L * P + 1, dtype=i64), lod=Z(P, dtype=torch.int8), dst_start=Z(P + 1, dtype=i64), n=5, means=Z(R, 3),
             shs=Z(R, K, 3), opacities=Z(R, 1), scales=Z(R, 3), rotations=Z(R, 4))
    a.update(bad)
    return lambda: _ops().lod_gather(*a.values(), out=out)


def _mlp(**bad):
    a = dict(features=Z(4, 8), weights=[Z(32, 12), Z(3, 32)], biases=[Z(32), Z(3)], embedding=Z(4))
    a.update(bad)
    return lambda: _ops().appearance_mlp(*a.values())


def _hash_levels():
    return _ops().hashgrid_levels(3, 2, 2, 8, 4, 1.5)


def _hex_layout():
    return _ops().hexplane_layout([2, 2, 2, 2], [1], 8)


def _graph():
    return _ops().KnnGraph(Z(4, 2, dtype=torch.int32), Z(5, dtype=torch.int32), Z(8, dtype=torch.int32))


def _features(**bad):
    a = dict(xys=Z(4, 2), depths=Z(4), radii=Z(4, dtype=torch.int32), conics=Z(4, 3), num_tiles_hit=Z(4, dtype=torch.int32), features=Z(4, 8),
             opacity=Z(4, 1), img_height=8, img_width=8, block_width=16)
    a.update(bad)
    return lambda: _ops().rasterize_features(*a.values())


small_out = [Z(4, 3), Z(4, 4, 3), Z(4, 1), Z(4, 3), Z(4, 4)]

# id -> (the call, the class, the substrings)
CASES = {
    # mesh: the device is asked first, so a CPU machine meets only that refusal
    "mesh/tsdf_fuse/non_tensor": (lambda: _ops().tsdf_fuse(([1.0], Z(4), None), Z(16), Z(1, 4, 4), Z(1, 4, 4)), RuntimeError,
                                  ["tsdf", "mesh ops run on the GPU only", "no CPU fallback"]),
    "mesh/tsdf_fuse/cpu": (lambda: _ops().tsdf_fuse((Z(4), Z(4), None), Z(16), Z(1, 4, 4), Z(1, 4, 4)), RuntimeError,
                           ["tsdf", "GPU only", "no CPU fallback"]),
    "mesh/soup/cpu": (lambda: _ops().marching_tetrahedra_soup(Z(2, 2, 2), 0.0, (0, 0, 0), (1, 1, 1)), RuntimeError,
                      ["volume", "GPU only", "no CPU fallback"]),
    "surface/depth_to_normal/cpu": (lambda: _ops().depth_to_normal(Z(4, 4), torch.eye(3)), RuntimeError, ["depth", "GPU only", "no CPU fallback"]),
    "surface/surfel_maps/non_tensor": (lambda: _ops().surfel_maps(None, torch.eye(3), torch.eye(3), 0.0), RuntimeError,
                                       ["allmap", "GPU only", "no CPU fallback"]),
    "surface/surface_reg/cpu": (lambda: _ops().surface_reg(Z(3, 4, 4), Z(3, 4, 4)), RuntimeError, ["a", "GPU only", "no CPU fallback"]),
    "bilagrid/slice/cpu": (lambda: _ops().bilagrid_slice(Z(1, 12, 2, 2, 2), Z(1, 4, 4, 2), Z(1, 4, 4, 3), Z(1, dtype=i64)), RuntimeError,
                           ["grids", "GPU only", "no CPU fallback"]),
    "bilagrid/tv/non_tensor": (lambda: _ops().bilagrid_tv([1.0]), RuntimeError, ["x", "GPU only", "no CPU fallback"]),
    "mcmc/relocation/cpu": (lambda: _ops().compute_relocation(Z(4), Z(4, 3), torch.ones(4, dtype=i64), Z(3, 3)), RuntimeError,
                            ["opacities", "GPU only", "no CPU fallback"]),
    "mcmc/perturb/cpu": (lambda: _ops().perturb_means_(Z(4, 3), Z(4, 3), Z(4, 4), Z(4), raw=True, noise_scale=1.0), RuntimeError,
                         ["means", "GPU only", "no CPU fallback"]),
    "mcmc/regularization/cpu": (lambda: _ops().mcmc_regularization(Z(4), Z(4, 3), 1.0, 1.0, raw=True), RuntimeError,
                                ["opacities", "GPU only", "no CPU fallback"]),
    "pvg/non_tensor": (lambda: _ops().pvg_motion(None, Z(4, 3), Z(4), Z(4), Z(4), 0.0, 1.0), ValueError, ["means must be [N, 3]"]),
    "pvg/shape": (lambda: _ops().pvg_motion(Z(4, 2), Z(4, 3), Z(4), Z(4), Z(4), 0.0, 1.0), ValueError, ["means must be [N, 3]", "[4, 2]"]),
    "pvg/cpu": (lambda: _ops().pvg_motion(Z(4, 3), Z(4, 3), Z(4), Z(4), Z(4), 0.0, 1.0), RuntimeError, ["means", "GPU only", "no CPU fallback"]),
    "envlight/cubemap/non_tensor": (lambda: _ops().cubemap_sample(None, Z(4, 3)), TypeError, ["texture", "tensor"]),
    "envlight/cubemap/dirs_non_tensor": (lambda: _ops().cubemap_sample(Z(6, 2, 2, 3), None), ValueError, ["directions", "[..., 3]"]),
    "envlight/cubemap/cpu": (lambda: _ops().cubemap_sample(Z(6, 2, 2, 3), Z(4, 3)), RuntimeError, ["base", "GPU only", "no CPU fallback"]),
    "envlight/blend/cpu": (lambda: _ops().envlight_blend(Z(3, 4, 4), Z(4, 4), Z(6, 2, 2, 3), torch.eye(3), 1.0, 1.0, 2.0, 2.0), RuntimeError,
                           ["rgb", "GPU only", "no CPU fallback"]),
    "segany/mask_stats/non_tensor": (lambda: _ops().segany_mask_stats([[1]]), TypeError, ["segany_mask_stats", "masks", "tensor"]),
    "segany/mask_stats/cpu": (lambda: _ops().segany_mask_stats(Z(2, 4, 4, dtype=torch.bool)), RuntimeError,
                              ["segany_mask_stats", "masks", "no CPU fallback"]),
    "segany/pack/cpu": (lambda: _ops().segany_pack_membership(Z(2, 4, 4, dtype=torch.uint8), Z(2, dtype=i64), Z(4, dtype=i64)), RuntimeError,
                        ["segany_pack_membership", "masks", "no CPU fallback"]),
    "segany/pair_labels/cpu": (lambda: _ops().segany_pair_labels(Z(4, 1, dtype=i64), Z(2, dtype=i64), Z(2, dtype=torch.bool)), RuntimeError,
                               ["segany_pair_labels", "bits", "no CPU fallback"]),
    "segany/loss_forward/non_tensor": (lambda: _ops().segany_loss_forward(None, (4, 4), Z(4, dtype=i64), Z(2, 4), Z(4, 4), Z(3), Z(4), None),
                                       TypeError, ["segany_loss_forward", "rendered", "tensor"]),
    "segany/loss/cpu": (lambda: _ops().segany_correspondence_loss(Z(4, 4, 4), (4, 4), Z(4, dtype=i64), Z(2, 4), Z(4, 4), Z(3), Z(4), None),
                        RuntimeError, ["segany_correspondence_loss", "rendered", "no CPU fallback"]),
    "spotless/mask/non_tensor": (lambda: _ops().spotless_mask(None, Z(4, 16), Z(4, 16), Z(16), Z(1)), TypeError, ["spotless_mask", "G", "tensor"]),
    "spotless/mask/cpu": (lambda: _ops().spotless_mask(Z(2, 2, 16), Z(4, 16), Z(4, 16), Z(16), Z(1)), RuntimeError,
                          ["spotless_mask", "G", "no CPU fallback"]),
    "spotless/mask_forward/cpu": (lambda: _ops().spotless_mask_forward(Z(2, 2, 16), Z(4, 16), Z(4, 16), Z(16), Z(1)), RuntimeError,
                                  ["spotless_mask", "G", "no CPU fallback"]),
    "spotless/error_stats/non_tensor": (lambda: _ops().spotless_error_stats(None, Z(3, 4, 4), Z(2), 8), TypeError,
                                        ["spotless_error_stats", "render", "tensor"]),
    "spotless/error_stats/cpu": (lambda: _ops().spotless_error_stats(Z(3, 4, 4), Z(3, 4, 4), Z(2), 8), RuntimeError,
                                 ["spotless_error_stats", "render", "no CPU fallback"]),
    "spotless/masked_l1/cpu": (lambda: _ops().spotless_masked_l1(Z(3, 4, 4), Z(3, 4, 4), Z(4, 4)), RuntimeError,
                               ["spotless_masked_l1", "render", "no CPU fallback"]),
    "spotless/masked_l1_forward/non_tensor": (lambda: _ops().spotless_masked_l1_forward([0.0], Z(3, 4, 4), Z(4, 4)), TypeError,
                                              ["spotless_masked_l1_forward", "render", "tensor"]),
    # glossy: types, shapes, the dtype, the device
    "glossy/non_tensor": (_glossy(opacity_dc=[0.0] * 4), TypeError, ["sh_view_opacities", "opacity_dc", "tensor"]),
    "glossy/shape/means": (_glossy(means=Z(4, 2)), ValueError, ["sh_view_opacities", "means must be [N, 3]", "4, 2"]),
    "glossy/shape/camera_center": (_glossy(camera_center=Z(4)), ValueError, ["sh_view_opacities", "camera_center", "3"]),
    "glossy/shape/opacity_dc": (_glossy(opacity_dc=Z(4, 2)), ValueError, ["sh_view_opacities", "opacity_dc", "[4, 1, 1]", "[4, 1]", "[4]"]),
    "glossy/shape/opacity_rest": (_glossy(opacity_rest=Z(5, 3, 1)), ValueError, ["sh_view_opacities", "opacity_rest", "[4, Kr, 1]"]),
    "glossy/degree": (_glossy(degree=5), ValueError, ["sh_view_opacities", "degree must be 0 .. 4, got 5"]),
    "glossy/dtype": (_glossy(opacity_rest=Z(4, 3, 1, dtype=f64)), NotImplementedError,
                     ["sh_view_opacities", "opacity_rest must be float32", "torch.float64"]),
    "glossy/cpu": (_glossy(), RuntimeError, ["sh_view_opacities", "means", "no CPU fallback"]),
    "glossy/forward/cpu": (lambda: _ops().sh_view_opacities_forward(1, Z(4, 3), Z(3), Z(4), Z(4, 3)), RuntimeError,
                           ["sh_view_opacities_forward", "means", "no CPU fallback"]),
    # lod: the same order
    "lod/select/levels": (_select(seg_start=[0, 1]), TypeError, ["lod_select", "seg_start", "tensor"]),
    "lod/select/levels_shape": (_select(seg_start=Z(11, dtype=i64)), ValueError, ["lod_select", "seg_start must be [L * 4 + 1]", "[11]"]),
    "lod/select/non_tensor": (_select(camera_center=[0.0, 0.0, 0.0]), TypeError, ["lod_select", "camera_center must be a tensor"]),
    "lod/select/shape": (_select(thresholds=torch.ones(3)), ValueError, ["lod_select", "thresholds must be [2], got [3]"]),
    "lod/select/dtype": (_select(prev_lod=Z(4, dtype=torch.int32)), NotImplementedError, ["lod_select", "prev_lod must be int8", "torch.int32"]),
    "lod/select/dtype_f64": (_select(transform=torch.eye(3, dtype=f64)), NotImplementedError, ["lod_select", "transform must be float32", "float64"]),
    "lod/select/filter_non_tensor": (_select(visibility_filter=True), TypeError, ["lod_select", "boxes3d must be a tensor"]),
    "lod/select/bool_prev_visible/cpu": (_select(prev_visible=torch.ones(4, dtype=torch.bool)), RuntimeError,
                                         ["lod_select", "seg_start", "no CPU fallback"]),
    "lod/select/cpu": (_select(), RuntimeError, ["lod_select", "seg_start", "no CPU fallback"]),
    "lod/gather/non_tensor": (_gather(lod=None), TypeError, ["lod_gather", "lod must be a tensor"]),
    "lod/gather/shape": (_gather(rotations=Z(8, 3)), ValueError, ["lod_gather", "rotations must be [8, 4], got [8, 3]"]),
    "lod/gather/dtype": (_gather(shs=Z(8, 4, 3, dtype=torch.float16)), NotImplementedError, ["lod_gather", "shs must be float32", "float16"]),
    "lod/gather/out_count": (_gather(out=small_out[:4]), ValueError, ["lod_gather", "five buffers"]),
    "lod/gather/out_shape": (_gather(out=small_out), ValueError, ["lod_gather", "out means must be [>= 5, 3]", "[4, 3]"]),
    "lod/gather/out_non_tensor": (_gather(out=[None] * 5), TypeError, ["lod_gather", "out means must be a tensor"]),
    "lod/gather/cpu": (_gather(), RuntimeError, ["lod_gather", "seg_start", "no CPU fallback"]),
    "hashgrid/levels": (lambda: _ops().hashgrid_encode(Z(4, 3), Z(8), object()), TypeError, ["hashgrid_encode", "levels"]),
    "hashgrid/non_tensor": (lambda: _ops().hashgrid_encode(np.zeros((4, 3), np.float32), Z(8), _hash_levels()), TypeError,
                            ["hashgrid_encode", "x", "tensor"]),
    "hashgrid/cpu": (lambda: _ops().hashgrid_encode(Z(4, 3), Z(_hash_levels().n_params), _hash_levels()), RuntimeError,
                     ["hashgrid_encode", "x must be", "no CPU fallback"]),
    "hexplane/layout": (lambda: _ops().hexplane_encode(Z(4, 3), 0.5, Z(8), np.zeros((2, 3)), object()), TypeError, ["hexplane_encode", "layout"]),
    "hexplane/non_tensor": (lambda: _ops().hexplane_encode(Z(4, 3), 0.5, None, np.zeros((2, 3)), _hex_layout()), TypeError,
                            ["hexplane_encode", "table", "tensor"]),
    "hexplane/cpu": (lambda: _ops().hexplane_encode(Z(4, 3), 0.5, Z(_hex_layout().total, 8), np.zeros((2, 3)), _hex_layout()), RuntimeError,
                     ["hexplane_encode", "x must be", "no CPU fallback"]),
    # knn and appearance: shapes first
    "knn/points/shape": (lambda: _ops().knn_points(Z(4, 3), Z(1, 4, 3)), ValueError, ["knn_points", "p1 and p2 must be [B, P, 3]", "(4, 3)"]),
    "knn/points/cpu": (lambda: _ops().knn_points(Z(1, 4, 3), Z(1, 4, 3)), RuntimeError, ["knn_points", "no CPU fallback"]),
    "knn/graph/non_tensor": (lambda: _ops().knn_graph([[0, 1]]), RuntimeError, ["knn_graph", "idx", "no CPU fallback"]),
    "knn/graph/cpu": (lambda: _ops().knn_graph(Z(4, 2, dtype=i64)), RuntimeError, ["knn_graph", "idx", "no CPU fallback"]),
    "knn/smooth/graph": (lambda: _ops().smooth_features(Z(4, 8), None), TypeError, ["smooth_features", "graph"]),
    "knn/smooth/non_tensor": (lambda: _ops().smooth_features(None, _graph()), RuntimeError, ["smooth_features", "features", "no CPU fallback"]),
    "knn/smooth/cpu": (lambda: _ops().smooth_features(Z(4, 8), _graph()), RuntimeError, ["smooth_features", "features", "no CPU fallback"]),
    "appearance/non_tensor": (_mlp(embedding=[0.0] * 4), TypeError, ["appearance_mlp", "embedding", "tensor"]),
    "appearance/shape/features": (_mlp(features=Z(8)), ValueError, ["appearance_mlp", "features must be [N, F]"]),
    "appearance/shape/weights": (_mlp(weights=[Z(32, 13), Z(3, 32)]), ValueError, ["appearance_mlp", "weights[0] must be [32, 12], got [32, 13]"]),
    "appearance/dtype": (_mlp(features=Z(4, 8, dtype=torch.float16)), NotImplementedError, ["appearance_mlp", "float16"]),
    "appearance/cpu": (_mlp(), RuntimeError, ["appearance_mlp", "features", "GPU", "no CPU fallback"]),
    "features/block_width": (_features(block_width=12), NotImplementedError, ["block_width"]),
    "features/shape": (_features(features=Z(5, 8)), ValueError, ["features must be [N, D]", "(5, 8)"]),
    "features/cpu": (_features(), RuntimeError, ["GPU only", "no CPU fallback"]),
}


def _refusal(call):
    try:
        call()
    except Exception as e:                        # noqa: BLE001 (the class is what is recorded)
        return type(e).__name__, str(e)
    return None, None


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_recorded_cases_are_the_cases_here(recorded):
    assert set(recorded) == set(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_refusal(case, recorded):
    call, cls, parts = CASES[case]
    assert recorded[case]["class"] == cls.__name__, "the class recorded before the move"
    assert all(p in recorded[case]["message"] for p in parts), "the substrings are taken from the recorded text"
    with pytest.raises(cls) as e:
        call()
    assert type(e.value) is cls
    missing = [p for p in parts if p not in str(e.value)]
    assert not missing, f"{case}: {str(e.value)!r} lacks {missing}"


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    rows = {}
    for case in sorted(CASES):
        name, text = _refusal(CASES[case][0])
        rows[case] = {"class": name, "message": text}
    with open(GOLDEN, "w") as f:
        json.dump(rows, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rows)} refusals in {GOLDEN}")

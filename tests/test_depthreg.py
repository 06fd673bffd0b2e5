"""The depth-regularisation route without a GPU: the CPU path of `ops.depth_loss`, the arithmetic of both plug-in metrics
(`gspl_amd.depthreg`) and `DepthMap` against tests/golden/ref_depthreg.npz — results of the reference's unedited
`HasInverseDepthMetricsModule`, `DepthMetricsModule` and `DepthMap`, recorded in float64 by tests/golden/make_depthreg_golden.py —
and the op's refusals."""
import json
import os
import pickle
import types

import numpy as np
import pytest
import torch

import gspl_amd  # noqa: F401
from gspl_amd import _lib as L
from gspl_amd import depthreg, ops

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_depthreg.npz"))
T = lambda name: torch.from_numpy(GOLDEN[name])
KINDS, NORMS, MASKS = ("l1", "l2"), ("none", "minmax", "median", "mean"), ("none", "gt", "pixel", "both")
CAMERA = torch.zeros(1)      # batch[0]: only its `.device` is read


def _close(got, name, tol=1e-12):
    ref = GOLDEN[name]
    got = got.detach().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (name, got.shape, ref.shape, got.dtype)
    assert float(np.abs(got - ref).max()) <= tol * max(1.0, float(np.abs(ref).max())), name


@pytest.mark.parametrize("masks", MASKS)
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_cpu_op_and_plugin_equal_the_reference_module(kind, norm, masks):
    gt_mask = T("gt_mask") if masks in ("gt", "both") else None
    pixel_mask = T("pixel_mask") if masks in ("pixel", "both") else None
    median = T("median") if norm == "median" else None
    pred = T("pred").requires_grad_(True)
    loss = ops.depth_loss(pred, T("gt"), kind, None if norm == "none" else norm, median, gt_mask, pixel_mask)
    assert loss.shape == () and loss.dtype == torch.float64
    loss.backward()
    _close(loss, f"has_{kind}_{norm}_{masks}")
    _close(pred.grad, f"has_{kind}_{norm}_{masks}_grad")

    config = depthreg.HipHasInverseDepthMetrics(depth_loss_type=kind, depth_normalized=norm == "minmax", depth_median_normalization=norm == "median",
                                                depth_mean_normalization=norm == "mean", depth_output_key="hard_inverse_depth")
    pred = T("pred").requires_grad_(True)
    batch = (CAMERA, ("name", T("gt_image"), pixel_mask), depthreg.DepthMap(depth=T("gt"), median=median, mask=gt_mask))
    loss = depthreg.inverse_depth_metric(config, batch, {"hard_inverse_depth": pred[None]})
    loss.backward()
    _close(loss, f"has_{kind}_{norm}_{masks}")
    _close(pred.grad, f"has_{kind}_{norm}_{masks}_grad")


@pytest.mark.parametrize("kind", KINDS)
def test_depth_metric_equals_the_reference_module(kind):
    pred = T("pred").requires_grad_(True)
    loss = depthreg.depth_metric(depthreg.HipDepthMetrics(depth_loss_type=kind), (CAMERA, None, (T("gt"), T("gt_mask"))), {"exp_depth": pred[None]})
    loss.backward()
    _close(loss, f"depth_{kind}")
    _close(pred.grad, f"depth_{kind}_grad")
    none = depthreg.depth_metric(depthreg.HipDepthMetrics(), (CAMERA, None, None), {})
    assert float(none) == 0.0 and float(depthreg.inverse_depth_metric(depthreg.HipHasInverseDepthMetrics(), (CAMERA, None, None), {})) == 0.0


def test_weight_schedule_and_logged_entries():
    scheduler = depthreg.WeightScheduler(init=0.7, final_factor=0.05, max_steps=1000)
    for config, name in ((depthreg.HipHasInverseDepthMetrics(depth_loss_weight=scheduler, depth_output_key="hard_inverse_depth"), "has"),
                         (depthreg.HipDepthMetrics(depth_loss_weight=scheduler), "depth")):
        weights = [depthreg.get_weight(config, int(s)) for s in GOLDEN["steps"]]
        assert weights == GOLDEN[f"{name}_weights"].tolist()      # the same expression: the same bits
        image_info = ("name", T("gt_image"), T("pixel_mask"))
        outputs = {"hard_inverse_depth": T("pred")[None], "exp_depth": T("pred")[None]}
        if name == "has":
            term = depthreg.inverse_depth_metric(config, (CAMERA, image_info, depthreg.DepthMap(depth=T("gt"), mask=T("gt_mask"))), outputs)
        else:
            term = depthreg.depth_metric(config, (CAMERA, image_info, (T("gt"), T("gt_mask"))), outputs)
        for stage, weight in (("train", depthreg.get_weight(config, 250)), ("validate", None)):
            ref = json.loads(str(GOLDEN[f"{name}_{stage}"]))
            own = ("d_reg", "d_w")
            # the photometric part is the reference's own VanillaMetricsImpl: its entries are taken as recorded
            basic = ({k: v for k, v in ref["metrics"].items() if k not in own}, {k: v for k, v in ref["prog_bar"].items() if k not in own})
            photometric = ref["metrics"]["loss"] - ref["metrics"]["d_reg"]
            basic[0]["loss"] = torch.tensor(photometric, dtype=torch.float64)
            metrics, prog_bar = depthreg.add_depth_term(basic, term, weight)
            assert sorted(metrics) == sorted(ref["metrics"]) and prog_bar == ref["prog_bar"]
            assert abs(float(metrics["d_reg"]) - ref["metrics"]["d_reg"]) <= 1e-12
            assert abs(float(metrics["loss"]) - ref["metrics"]["loss"]) <= 1e-12
            if weight is not None:
                assert metrics["d_w"] == ref["metrics"]["d_w"]


def test_get_predicted_depth_renders_the_depth_camera_for_the_depth_type_alone():
    config = depthreg.HipHasInverseDepthMetrics(depth_output_key="hard_inverse_depth")
    calls = []

    def renderer(camera, model, bg, render_types):
        calls.append({"camera": list(camera), "model": model, "bg": bg.tolist(), "bg_dtype": str(bg.dtype), "render_types": render_types})
        return {"hard_inverse_depth": T("pred")[None]}
    pl_module = types.SimpleNamespace(device=torch.device("cpu"), renderer=renderer)
    depth_camera = types.SimpleNamespace(to_device=lambda device: ("camera on", str(device)))
    batch = (CAMERA, None, depthreg.DepthMap(depth=T("gt"), camera=depth_camera))
    got = depthreg.get_predicted_depth(config, pl_module, "model", batch, {"render": T("render")})
    assert got["hard_inverse_depth"] is not None and calls == [json.loads(str(GOLDEN["has_rendered"]))]
    kept = {"hard_inverse_depth": T("pred")[None]}
    assert depthreg.get_predicted_depth(config, pl_module, "model", batch, kept) is kept and len(calls) == 1
    assert depthreg.get_predicted_depth(config, pl_module, "model", (CAMERA, None, None), {"render": None})["render"] is None and len(calls) == 1


def test_depth_map_equals_the_reference_class():
    scale, offset = float(GOLDEN["dm_scale"]), float(GOLDEN["dm_offset"])
    a = depthreg.DepthMap.create(T("dm_float"), scale, offset)
    assert a.scale is None and a.offset is None and a.median is None and a.mask is None and a.camera is None
    _close(a.get(), "dm_create_float", 0.0)
    assert float(a.get().min()) == 0.0                      # the clamp is exercised
    a.media_normalize()
    _close(a.median, "dm_create_float_median", 0.0)
    _close(a.get(), "dm_create_float_normalized", 0.0)
    _close(depthreg.DepthMap.create(GOLDEN["dm_u16"], scale, offset).get(), "dm_create_u16_as_float", 0.0)
    c = depthreg.DepthMap.create(GOLDEN["dm_u16"], scale, offset, in_uint16=True)
    assert c.depth.dtype == np.uint16 and c.scale == scale and c.offset == offset
    _close(c.get_scaled(), "dm_u16_get_scaled", 0.0)
    _close(c.get(), "dm_u16_get", 0.0)
    c.media_normalize()
    assert c.depth.dtype == np.uint16
    _close(c.median, "dm_u16_median", 0.0)
    _close(c.get(), "dm_u16_get_normalized", 0.0)
    with pytest.raises(AssertionError):
        depthreg.DepthMap.create(GOLDEN["dm_float"], scale, offset, in_uint16=True)
    assert not hasattr(depthreg, "cv2")


def test_refusals():
    pred, gt = T("pred"), T("gt")
    with pytest.raises(NotImplementedError, match="l1\\+ssim is not built.*torchmetrics"):
        ops.depth_loss(pred, gt, "l1+ssim")
    with pytest.raises(NotImplementedError, match="kind must be 'l1' or 'l2'"):
        ops.depth_loss(pred, gt, "kl")
    with pytest.raises(ValueError, match="normalize must be"):
        ops.depth_loss(pred, gt, "l1", "max")
    with pytest.raises(TypeError, match="depth_loss: pred must be a tensor"):
        ops.depth_loss(pred.numpy(), gt)
    with pytest.raises(ValueError, match=r"depth_loss: pred must be \[H, W\]"):
        ops.depth_loss(pred[None], gt)
    with pytest.raises(ValueError, match="depth_loss: gt must be"):
        ops.depth_loss(pred, gt[:-1])
    with pytest.raises(ValueError, match="`median` goes with normalize='median'"):
        ops.depth_loss(pred, gt, "l1", "median")
    with pytest.raises(ValueError, match="`median` goes with normalize='median'"):
        ops.depth_loss(pred, gt, "l1", None, 2.0)
    with pytest.raises(ValueError, match="depth_loss: gt_mask must hold"):
        ops.depth_loss(pred, gt, gt_mask=gt[:-1])
    with pytest.raises(RuntimeError, match="depth_loss: gt is on meta, pred on cpu"):
        ops.depth_loss(pred, gt.to("meta"))
    with pytest.raises(RuntimeError, match="depth_loss: pixel_mask is on meta, pred on cpu"):
        ops.depth_loss(pred, gt, pixel_mask=T("pixel_mask").to("meta"))
    for name, who in (("HipHasInverseDepthMetrics", "HipHasInverseDepthMetrics"), ("HipDepthMetrics", "HipDepthMetrics")):
        with pytest.raises(NotImplementedError, match=f"{who}.*l1\\+ssim.*torchmetrics"):
            depthreg.check_loss_type(who, "l1+ssim")
        with pytest.raises(NotImplementedError, match="must be 'l1' or 'l2'"):
            depthreg.check_loss_type(who, "kl")


def test_plugins_are_importable_picklable_and_name_the_reference_class():
    for cls, ref in ((depthreg.HipHasInverseDepthMetrics, "internal.metrics.inverse_depth_metrics.HasInverseDepthMetrics"),
                     (depthreg.HipDepthMetrics, "internal.metrics.depth_metrics.DepthMetrics")):
        cfg = cls(depth_loss_type="l2", depth_loss_weight=depthreg.WeightScheduler(init=0.5))
        assert pickle.loads(pickle.dumps(cfg)) == cfg           # stored in checkpoint hparams by the reference
        if depthreg._VanillaMetrics is None:
            with pytest.raises(RuntimeError, match=ref.replace(".", r"\.")):
                cfg.instantiate()
    defaults = depthreg.HipHasInverseDepthMetrics()
    assert (defaults.depth_loss_type, defaults.depth_loss_ssim_weight, defaults.depth_normalized, defaults.depth_median_normalization,
            defaults.depth_mean_normalization, defaults.depth_output_key) == ("l1", 0.2, False, False, False, "inverse_depth")
    assert depthreg.HipDepthMetrics().predicted_depth_key == "exp_depth"
    assert depthreg.WeightScheduler() == depthreg.WeightScheduler(init=1.0, final_factor=0.01, max_steps=30_000)
    m = pickle.loads(pickle.dumps(depthreg.DepthMap(depth=T("gt"), median=1.5)))
    assert torch.equal(m.depth, T("gt")) and m.median == 1.5


def test_header_declares_the_entry_points_and_constants():
    for name in ("gspl_depth_loss_workspace_bytes", "gspl_depth_loss_fwd", "gspl_depth_loss_bwd"):
        assert name in L.exported_symbols()
    assert (L.GSPL_DEPTH_LOSS_L1, L.GSPL_DEPTH_LOSS_L2) == (0, 1)
    assert (L.GSPL_DEPTH_NORM_NONE, L.GSPL_DEPTH_NORM_MINMAX, L.GSPL_DEPTH_NORM_MEDIAN, L.GSPL_DEPTH_NORM_MEAN) == (0, 1, 2, 3)
    assert L.ABI_VERSION == 39

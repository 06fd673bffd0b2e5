"""
make_depthreg_golden.py — generates tests/golden/ref_depthreg.npz by IMPORTING the reference's own, unedited
`internal.metrics.inverse_depth_metrics`, `internal.metrics.depth_metrics` and `DepthMap` of
`internal.dataparsers.estimated_depth_colmap_dataparser` where its tree is present, behind the test-only stand-ins of
tests/lightning_standin.py for the packages those modules import and this container lacks (`torchmetrics`, `cv2`, `lightning`), and
running them in float64 on the CPU.

Run from the repo root, in a process of its own:   python tests/golden/make_depthreg_golden.py <path to the reference tree>
Its output is committed (inputs and recorded results only); no test runs this script.

Fixture (ref_depthreg.npz), float64 unless noted
  pred, gt [13, 11] (0.05 .. 3.05), gt_mask [13, 11] (a weight map with zeros), pixel_mask [13, 11] bool, median (of gt's positive values)
  render, gt_image [3, 13, 11]            the images of the photometric part of get_train_metrics / get_validate_metrics
  has_<kind>_<norm>_<masks>, ..._grad     HasInverseDepthMetricsModule.get_inverse_depth_metric and autograd's gradient for `pred`;
                                          kind l1 | l2, norm none | minmax | median | mean, masks none | gt | pixel | both
  depth_<kind>, ..._grad                  DepthMetricsModule.get_inverse_depth_metric with (gt, gt_mask)
  steps [5] int64, has_weights, depth_weights [5]      get_weight(step), WeightScheduler(init=0.7, final_factor=0.05, max_steps=1000)
  has_train, has_validate, depth_train, depth_validate  JSON: the metrics' names with their values, and the progress-bar dict
  has_rendered                            JSON: the arguments of the renderer call get_predicted_depth makes when the outputs lack the key
  dm_*                                    DepthMap: inputs (a float32 map with negative values, a uint16 map, scale, offset) and what
                                          create / get / get_scaled / media_normalize leave, both forms
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
H, W = 13, 11
KINDS, NORMS, MASKS = ("l1", "l2"), ("none", "minmax", "median", "mean"), ("none", "gt", "pixel", "both")


def inputs():
    g = torch.Generator().manual_seed(29)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    pred, gt = r(H, W) * 3 + 0.05, r(H, W) * 3 + 0.05
    gt_mask = (r(H, W) > 0.2).double() * (0.5 + r(H, W))
    pixel_mask = r(H, W) > 0.3
    return dict(pred=pred, gt=gt, gt_mask=gt_mask, pixel_mask=pixel_mask, median=torch.median(gt[gt > 0]), render=r(3, H, W), gt_image=r(3, H, W))


def main(reference):
    for p in (reference, os.path.join(ROOT, "tests"), ROOT):
        sys.path.insert(0, p)
    import lightning_standin
    lightning_standin.install()
    from internal.metrics.inverse_depth_metrics import HasInverseDepthMetrics, WeightScheduler
    from internal.metrics.depth_metrics import DepthMetrics, WeightScheduler as DepthWeightScheduler
    from internal.dataparsers.estimated_depth_colmap_dataparser import DepthMap

    x = inputs()
    out = {k: v.numpy() for k, v in x.items()}
    camera = torch.zeros(1)      # batch[0]: only its `.device` is read

    def module(config):
        m = config.instantiate()
        m.setup("fit", None)
        return m

    for kind in KINDS:
        for norm in NORMS:
            for masks in MASKS:
                m = module(HasInverseDepthMetrics(depth_loss_type=kind, depth_normalized=norm == "minmax", depth_median_normalization=norm == "median",
                                                  depth_mean_normalization=norm == "mean", depth_output_key="hard_inverse_depth"))
                data = DepthMap(depth=x["gt"], median=x["median"] if norm == "median" else None, mask=x["gt_mask"] if masks in ("gt", "both") else None)
                pred = x["pred"].clone().requires_grad_(True)
                batch = (camera, ("name", x["gt_image"], x["pixel_mask"] if masks in ("pixel", "both") else None), data)
                loss = m.get_inverse_depth_metric(batch, {"hard_inverse_depth": pred[None]})
                loss.backward()
                out[f"has_{kind}_{norm}_{masks}"], out[f"has_{kind}_{norm}_{masks}_grad"] = loss.detach().numpy(), pred.grad.numpy()
        m = module(DepthMetrics(depth_loss_type=kind))
        pred = x["pred"].clone().requires_grad_(True)
        loss = m.get_inverse_depth_metric((camera, None, (x["gt"], x["gt_mask"])), {"exp_depth": pred[None]})
        loss.backward()
        out[f"depth_{kind}"], out[f"depth_{kind}_grad"] = loss.detach().numpy(), pred.grad.numpy()

    steps = [0, 250, 1000, 1001, 5000]
    out["steps"] = np.asarray(steps, np.int64)
    has = module(HasInverseDepthMetrics(depth_loss_weight=WeightScheduler(init=0.7, final_factor=0.05, max_steps=1000), depth_output_key="hard_inverse_depth"))
    depth = module(DepthMetrics(depth_loss_weight=DepthWeightScheduler(init=0.7, final_factor=0.05, max_steps=1000)))
    out["has_weights"] = np.asarray([has.get_weight(s) for s in steps])
    out["depth_weights"] = np.asarray([depth.get_weight(s) for s in steps])
    # the validation's psnr / lpips are torchmetrics objects: here the stand-in's, so only their NAMES are recorded
    number = lambda v: float(v) if isinstance(v, (float, int, torch.Tensor)) else None
    record = lambda pair: json.dumps({"metrics": {k: number(v) for k, v in pair[0].items()}, "prog_bar": pair[1]}, sort_keys=True)
    image_info = ("name", x["gt_image"], x["pixel_mask"])
    outputs = {"render": x["render"], "hard_inverse_depth": x["pred"][None], "exp_depth": x["pred"][None]}
    has_batch = (camera, image_info, DepthMap(depth=x["gt"], mask=x["gt_mask"]))
    depth_batch = (camera, image_info, (x["gt"], x["gt_mask"]))
    out["has_train"] = np.asarray(record(has.get_train_metrics(None, None, 250, has_batch, outputs)))
    out["has_validate"] = np.asarray(record(has.get_validate_metrics(None, None, has_batch, outputs)))
    out["depth_train"] = np.asarray(record(depth.get_train_metrics(None, None, 250, depth_batch, outputs)))
    out["depth_validate"] = np.asarray(record(depth.get_validate_metrics(None, None, depth_batch, outputs)))

    # get_predicted_depth: the outputs lack the key and the batch carries a depth camera
    calls = []
    depth_camera = types.SimpleNamespace(to_device=lambda device: ("camera on", str(device)))

    def renderer(camera_, model, bg, render_types):
        calls.append({"camera": list(camera_), "model": model, "bg": bg.tolist(), "bg_dtype": str(bg.dtype), "render_types": render_types})
        return {"hard_inverse_depth": x["pred"][None]}
    pl_module = types.SimpleNamespace(device=torch.device("cpu"), renderer=renderer)
    got = has.get_predicted_depth(pl_module, "model", (camera, image_info, DepthMap(depth=x["gt"], camera=depth_camera)), {"render": x["render"]})
    assert got["hard_inverse_depth"] is not None and len(calls) == 1
    kept = {"hard_inverse_depth": x["pred"][None]}
    assert has.get_predicted_depth(pl_module, "model", has_batch, kept) is kept and len(calls) == 1
    out["has_rendered"] = np.asarray(json.dumps(calls[0], sort_keys=True))

    # DepthMap
    g = torch.Generator().manual_seed(31)
    dm_float = (torch.rand(6, 5, generator=g) * 4 - 0.5).numpy().astype(np.float32)
    dm_u16 = torch.randint(0, 65536, (6, 5), generator=g).numpy().astype(np.uint16)
    dm_u16[0, :2] = 0
    scale, offset = 2.75, -0.4
    out.update(dm_float=dm_float, dm_u16=dm_u16, dm_scale=np.asarray(scale), dm_offset=np.asarray(offset))
    a = DepthMap.create(torch.from_numpy(dm_float), scale, offset)
    out["dm_create_float"] = a.get().numpy().copy()
    a.media_normalize()
    out["dm_create_float_median"], out["dm_create_float_normalized"] = a.median.numpy(), a.get().numpy()
    b = DepthMap.create(dm_u16, scale, offset)
    out["dm_create_u16_as_float"] = b.get().numpy()
    c = DepthMap.create(dm_u16, scale, offset, in_uint16=True)
    assert c.depth.dtype == np.uint16 and c.scale == scale and c.offset == offset
    out["dm_u16_get_scaled"], out["dm_u16_get"] = c.get_scaled().numpy(), c.get().numpy()
    c.media_normalize()
    assert c.depth.dtype == np.uint16
    out["dm_u16_median"], out["dm_u16_get_normalized"] = c.median.numpy(), c.get().numpy()

    path = os.path.join(HERE, "ref_depthreg.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])

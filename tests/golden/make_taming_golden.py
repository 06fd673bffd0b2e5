"""
make_taming_golden.py — generates tests/golden/ref_taming.npz by IMPORTING the reference's own, unedited
internal/density_controllers/taming_3dgs_density_controller.py where its tree is present and calling `Taming3DGSUtils`' static methods,
and by running PIL's own `convert('L')` and `filter(ImageFilter.FIND_EDGES)` on the same images.

The reference module imports `lightning` (tests/lightning_standin.py stands in, as in the other workers), `gsplat` and `fused_ssim`
(gspl_amd.compat's stand-ins) and `torchvision.transforms`, which is not installed here: a test-only module with `ToPILImage` and
`ToTensor` by their documented rules stands in (a float [C, H, W] tensor is `mul(255).byte()`, channels last, into `Image.fromarray`; a
PIL image of bytes comes back as [C, H, W] float `div(255)`).

Run from the repo root, in a process of its own:   python tests/golden/make_taming_golden.py <path to the reference tree>
Its output is committed; no test runs this script.

Fixture (ref_taming.npz)
  count/cfg [K, 5] float64, count/mode [K] (0 multiplier, 1 final_count), count/len [K], count/values [sum len] int64
      `get_count_array(start_count, multiplier, densify_until_iter, densify_from_iter, densification_interval, mode)`
  row/<name>             the input row (float32 or int32), one per case of tests/test_taming.py
  median/<name> [1]      `torch.median(v[v > 0])` as `normalize` forms it (absent for the row without a valid entry)
  norm/<name>            `normalize(7.5, row.clone())` (zeros for the row without a valid entry)
  lossmap/render, gt [3, H, W], lossmap/edges [H, W], lossmap/out [H, W]     `get_loss_map` with mse 50, edge 50 (the defaults)
  img/<name> [3, H, W] uint8, edges/<name> [H, W] float32 = `get_edges(img / 255.)[0]`, pil_l/<name>, pil_edges/<name> [H, W] uint8
  imgf/floats [3, H, W] float32 off the byte grid, edges/floats, pil_edges/floats the same for it (PIL fed through the stand-in ToPILImage)
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)


def install_torchvision_stand_in():
    from PIL import Image

    class ToPILImage:
        def __call__(self, pic):
            assert pic.dim() == 3 and pic.is_floating_point()
            a = pic.mul(255).byte().permute(1, 2, 0).numpy()
            return Image.fromarray(a[:, :, 0], mode="L") if a.shape[2] == 1 else Image.fromarray(a, mode="RGB")

    class ToTensor:
        def __call__(self, img):
            a = np.array(img)
            if a.ndim == 2:
                a = a[:, :, None]
            return torch.from_numpy(a).permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    tv, tt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tt.ToPILImage, tt.ToTensor = ToPILImage, ToTensor
    tv.transforms = tt
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tt
    return ToPILImage


def rows(g):
    sub = torch.tensor([1e-45, 3e-45, 1e-40, 0.0, 5e-39, -1e-40], dtype=torch.float32)
    nan, inf = float("nan"), float("inf")
    return {
        "n1": torch.tensor([0.0, -2.0, 3.5, nan]),
        "n2_lower": torch.tensor([4.0, 0.0, 2.0]),
        "even": torch.rand(40, generator=g) + 0.01,
        "odd": torch.cat([torch.rand(41, generator=g) * 100, torch.tensor([-1.0, 0.0, nan])]),
        "all_equal": torch.full((17,), 0.3),
        "ties": torch.tensor([1.0, 2.0, 2.0, 2.0, 2.0, 3.0, 0.0, 2.0, 5.0, 1.0]),
        "none_valid": torch.tensor([0.0, -1.0, nan, -0.0, -inf, nan]),
        "with_inf": torch.tensor([inf, 1.0, inf, inf, 2.0, 0.0]),
        "subnormals": sub,
        "i32": torch.tensor([0, 7, -3, 2, 9, 9, 1, 0, 2147483647], dtype=torch.int32),
    }


def images(g):
    levels = torch.arange(768) % 256
    all_levels = torch.stack([levels[torch.randperm(768, generator=g)] for _ in range(3)]).reshape(3, 32, 24).to(torch.uint8)
    assert all(len(set(all_levels[c].reshape(-1).tolist())) == 256 for c in range(3))
    out = {"levels": all_levels}
    for name, (h, w) in {"1x1": (1, 1), "1x7": (1, 7), "2x5": (2, 5), "3x3": (3, 3)}.items():
        out[name] = torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)
    return out


def main(reference):
    for p in (reference, TESTS, ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    import lightning_standin
    lightning_standin.install()
    import gspl_amd  # noqa: F401
    from gspl_amd import renderers  # noqa: F401   (installs the stand-ins of gspl_amd.compat)
    ToPILImage = install_torchvision_stand_in()
    from PIL import ImageFilter
    from internal.density_controllers.taming_3dgs_density_controller import ScoreCoefficients, Taming3DGSUtils as U

    out = {}
    configs = [(1000, 20, 15000, 500, 500, "multiplier"), (182686, 15.0, 15000, 500, 500, "multiplier"), (5000, 2.5, 30000, 1000, 300, "multiplier"),
               (1000, 250000, 15000, 500, 500, "final_count"), (100000, 60000, 15000, 500, 100, "final_count"), (777, 0.5, 7000, 600, 250, "multiplier")]
    values = [U.get_count_array(*c) for c in configs]
    out["count/cfg"] = np.array([c[:5] for c in configs], dtype=np.float64)
    out["count/mode"] = np.array([0 if c[5] == "multiplier" else 1 for c in configs], dtype=np.int64)
    out["count/len"] = np.array([len(v) for v in values], dtype=np.int64)
    out["count/values"] = np.array([x for v in values for x in v], dtype=np.int64)
    assert values[4][-1] <= 100000 and values[5][0] == 777          # budgets below the start count: the curve stays at the start

    g = torch.Generator().manual_seed(20262)
    for name, row in rows(g).items():
        out[f"row/{name}"] = row.numpy().copy()
        valid = row[row > 0].to(torch.float32)
        if valid.numel():
            out[f"median/{name}"] = torch.median(valid).reshape(1).numpy()
        out[f"norm/{name}"] = U.normalize(7.5, row.clone()).numpy()

    H, W = 13, 21
    render, gt, edges = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g), torch.rand(H, W, generator=g)
    out["lossmap/render"], out["lossmap/gt"], out["lossmap/edges"] = render.numpy(), gt.numpy(), edges.numpy()
    out["lossmap/out"] = U.get_loss_map(render, gt, ScoreCoefficients(), edges).numpy()

    for name, img in images(g).items():
        out[f"img/{name}"] = img.numpy()
        out[f"edges/{name}"] = U.get_edges(img.float() / 255.)[0].numpy()
        pil = ToPILImage()(img.float() / 255.)
        assert np.array_equal(np.array(pil), img.permute(1, 2, 0).numpy()), "the / 255, * 255 round trip is not the identity"
        grey = pil.convert("L")
        out[f"pil_l/{name}"] = np.array(grey)
        out[f"pil_edges/{name}"] = np.array(grey.filter(ImageFilter.FIND_EDGES))
    floats = torch.rand(3, 9, 11, generator=g)
    floats[0, 0, 0], floats[1, 0, 1], floats[2, 4, 4] = 1.0, 0.0, 254.999 / 255
    out["imgf/floats"] = floats.numpy()
    out["edges/floats"] = U.get_edges(floats)[0].numpy()
    out["pil_edges/floats"] = np.array(ToPILImage()(floats).convert("L").filter(ImageFilter.FIND_EDGES))

    path = os.path.join(HERE, "ref_taming.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])

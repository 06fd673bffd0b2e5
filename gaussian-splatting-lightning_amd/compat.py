"""Import shims for the reference's un-vendored native packages that this package replaces.

Besides the small helpers below (`simple_knn`, `fused_ssim`, and `fused_bilagrid` — the bilateral-grid processor's slice and TV
loss, bound late to `gspl_amd.bilagrid`), `install()` registers stand-ins for the rasterizer
packages themselves — `diff_gaussian_rasterization`, Taming 3DGS's `diff_accel_gaussian_rasterization`, 2DGS's
`diff_surfel_rasterization` and the yzslab `gsplat` fork — under the module paths and function names the
reference imports (internal/renderers/vanilla_renderer.py:4, gsplat_renderer.py:2-4, gsplat_v1_renderer.py:8-20,
pypreprocess_gsplat_renderer.py:1-2, gsplat_hit_pixel_count_renderer.py:5, internal/optimizers.py:34 ...), each bound to the HIP
op of `gspl_amd.ops` with the same signature.  With them the reference's OWN renderer classes (`VanillaRenderer`,
`GSPlatRenderer`, `GSplatV1Renderer`, the research renderers built on their static helpers) run unedited on the HIP kernels; the
`Hip*` plugins of `gspl_amd.renderers` remain the faster route (fused calls, list-only binning, channels-first images).
`gsplat.utils.depth_to_normal` (internal/metrics/normal_reg.py:3) is served by `ops.depth_to_normal` with the semantics of the
published gsplat `utils.py`; parity with the fork's own build of it is unpinned (there is no ROCm build to compare against).
Functions of the fork that are not built (`compute_relocation`, `rasterize_to_vis_aware_weights`) are left out: importing them
raises ImportError as it would without the package.
For the Periodic Vibration Gaussian route (internal/renderers/periodic_vibration_gaussian_renderer.py:9,
internal/model_components/envlight.py:2) two more stand-ins exist, each with the ONE function that route calls: `nvdiffrast.torch`
with `texture` — cube maps only (tex [1, 6, R, R, 3], uv [B, H, W, 3], filter_mode='linear', boundary_mode='cube', no mip-maps, no
gradient for uv), served by `ops.cubemap_sample` with the published OpenGL / nvdiffrast semantics; parity with nvdiffrast's own build
is unpinned; everything else of nvdiffrast (rasterisation, 2D textures, antialiasing) is NOT built and raises — and `kornia.utils` with
`create_meshgrid` in plain torch; nothing else of kornia is built.  With them the reference's own PVG renderer and `EnvLight` import
unedited (the call `EnvLight.forward` makes is tested through the stand-in on the GPU; a whole forward pass of the reference's renderer on
them is untested); `HipPeriodicVibrationGaussianRenderer` is the route that is tested end to end.
For the SegAnyGS route (internal/segany_splatting.py:14,273) and the appearance-similarity regulariser
(internal/metrics/appearance_feature_similarity_regularization_metrics.py:8,70-74) `pytorch3d.ops` exists with the ONE function they
call, `knn_points`, bound late to `ops.knn_points`: 3-D clouds, K <= 32, no `lengths`, the published semantics with neighbours
ordered by (d^2, index); parity with pytorch3d's own build is unpinned (there is none for ROCm here).  Nothing else of pytorch3d is
built: `pytorch3d.ops.iou_box3d` (the partition-LoD renderer's) and everything else keep raising ImportError.  With it
`SegAnySplatting` imports unedited; `gspl_amd.segany.use_hip_smoothing` then replaces its per-step gather by the fused op.
For the SWAG route (internal/models/swag_model.py:72-78) `tinycudann` exists with ONE class, `Encoding(n_input_dims, encoding_config,
seed=1337, dtype=None)` (`gspl_amd.hashgrid.Encoding`), for the grid encodings only: otype `HashGrid`, `DenseGrid`, or `Grid` with type
`Hash` / `Dense`; 2 or 3 input dimensions, 1, 2, 4 or 8 features per level, up to 32 levels, linear interpolation, a float32 table
(`.params`, uniform in [-1e-4, 1e-4] from the seed) and float32 output, served by `ops.hashgrid_encode` with the published rules of
tiny-cuda-nn's grid; parity with its own build is unpinned (there is none for ROCm).  Any other otype (Frequency, SphericalHarmonics,
Identity, ...) or option (Smoothstep, half precision, Tiled) raises NotImplementedError naming it.  `Network`,
`NetworkWithInputEncoding` and the fused MLPs are NOT built and absent, so `from tinycudann import Network` keeps raising ImportError:
the reference's renderers that need them (`NetworkFactory(tcnn=True)`) stay unserved, while SWAG's `NetworkFactory(tcnn=False)` MLP is
plain torch.nn.  With it the reference's own `SWAGModel` / `SWAGRenderer` construct unedited; `HipSWAGRenderer` is the tested route.

The reference imports them by their own module names inside functions, e.g.
`from simple_knn._C import distCUDA2` (internal/models/vanilla_gaussian.py:122) or `from fused_ssim import fused_ssim`
(internal/metrics/vanilla_metrics.py:36).  `install()` registers stand-in
modules under those names — only for packages that are NOT importable — so that the reference runs unedited once
`gspl_amd.renderers` has been imported (which the `--model.renderer gspl_amd.renderers.<Name>` option does while the
configuration is parsed, long before the model is initialised from a point cloud).
"""
from __future__ import annotations

import importlib.util
import sys
import types


def _missing(name: str) -> bool:
    if name in sys.modules:
        return False
    try:
        return importlib.util.find_spec(name) is None
    except (ImportError, ValueError):
        return True


def _late(name: str, module: str = "ops"):
    """Call-time binding to `gspl_amd.<module>.<name>` (so that it can be looked up — or replaced in a test — after install)."""
    def fn(*args, **kwargs):
        return getattr(importlib.import_module(f"{__package__}.{module}"), name)(*args, **kwargs)
    fn.__name__ = fn.__qualname__ = name
    fn.__doc__ = f"gspl_amd.{module}.{name} (HIP)"
    return fn


def _isect_tiles_tile_based_culling(means2d, radii, depths, conics, opacities, tile_size, tile_width, tile_height, packed=False,
                                    n_cameras=1, camera_ids=None, gaussian_ids=None):
    """The fork's `isect_tiles_tile_based_culling` as the reference calls it (gsplat_v1_renderer.py:497-510): a (tile, Gaussian)
    pair is listed only if the Gaussian can reach alpha >= 1/255 in the tile.  Served by the list-only two-level binning, which
    produces the sorted lists directly: the `isect_ids` it returns is an empty tensor that carries the tile offsets to
    `isect_offset_encode_tile_based_culling` (the reference hands it straight over, :511-517)."""
    import torch
    from . import ops
    if packed or camera_ids is not None or gaussian_ids is not None or n_cameras not in (None, 1):
        raise NotImplementedError("one camera per call, unpacked (what the reference uses)")
    flat, offsets = ops.bin_gaussians(means2d.reshape(-1, 2), depths.reshape(-1), radii.reshape(-1), int(tile_height) * int(tile_size),
                                      int(tile_width) * int(tile_size), int(tile_size), conics=conics.reshape(-1, 3),
                                      opacities=opacities.reshape(-1))
    carrier = torch.empty((0,), dtype=torch.int64, device=flat.device)
    carrier._gspl_offsets = offsets.reshape(1, int(tile_height), int(tile_width))
    return None, carrier, flat


def _isect_offset_encode_tile_based_culling(isect_ids, flatten_ids, n_cameras, tile_width, tile_height):
    offsets = getattr(isect_ids, "_gspl_offsets", None)
    if offsets is None:
        raise ValueError("isect_ids must come from gspl_amd's isect_tiles_tile_based_culling")
    return offsets, flatten_ids


def _rasterize_to_pixels_fork(*args, **kwargs):
    """The fork's rasterize_to_pixels ALWAYS leaves `means2d.has_hit_any_pixels` behind (gsplat_v1_renderer.py:287 reads it
    unconditionally); ops.rasterize_to_pixels does so on request."""
    from . import ops
    kwargs.setdefault("track_hits", True)
    return ops.rasterize_to_pixels(*args, **kwargs)


def _depth_to_normal(depths, camtoworlds, Ks, z_depth=True):
    """gsplat's `utils.depth_to_normal` as published: depths [..., H, W, 1], camtoworlds [..., 4, 4], Ks [..., 3, 3] -> normals
    [..., H, W, 3] in world space, zero on the one-pixel border.  Pixel centres lie at +0.5 (`ops.gsplat_rays`); z_depth=False means
    `depths` are distances along the normalised rays.  One `ops.depth_to_normal` launch per image, A built on the device without a
    read-back; the gradient reaches `depths` only.  Parity with the yzslab fork's build is unpinned: these are the published
    semantics, which the reference's call site (internal/metrics/normal_reg.py:29-33) relies on."""
    import torch
    from . import ops
    if depths.dim() < 3 or depths.shape[-1] != 1:
        raise ValueError(f"depths must be [..., H, W, 1], got {tuple(depths.shape)}")
    H, W = int(depths.shape[-3]), int(depths.shape[-2])
    lead = tuple(depths.shape[:-3])
    d = depths.reshape(-1, H, W)
    c2w = camtoworlds.expand(*lead, 4, 4).reshape(-1, 4, 4)
    Ks = Ks.expand(*lead, 3, 3).reshape(-1, 3, 3)
    if d.shape[0] == 0:
        return depths.new_zeros((*lead, H, W, 3))
    maps = [ops.depth_to_normal(d[i], ops.gsplat_rays(c2w[i], Ks[i]).to(d.dtype), normalize_rays=not z_depth) for i in range(d.shape[0])]
    return torch.stack(maps).reshape(*lead, H, W, 3)


def _texture(tex, uv, uv_da=None, mip_level_bias=None, mip=None, filter_mode="auto", boundary_mode="wrap", max_mip_level=None):
    """`nvdiffrast.torch.texture` for the one form the reference uses (envlight.py:20): a cube map tex [1, 6, R, R, 3] sampled along
    uv [B, H, W, 3] with filter_mode='linear' and boundary_mode='cube' -> [B, H, W, 3].  Anything else raises NotImplementedError."""
    from . import ops
    if uv_da is not None or mip_level_bias is not None or mip is not None or max_mip_level is not None:
        raise NotImplementedError("mip-mapped texture sampling is not built")
    if filter_mode != "linear" or boundary_mode != "cube":
        raise NotImplementedError(f"only filter_mode='linear' with boundary_mode='cube' is built, got {filter_mode!r} / {boundary_mode!r}")
    if tex.dim() != 5 or tex.shape[0] != 1 or tex.shape[1] != 6 or tex.shape[2] != tex.shape[3]:
        raise NotImplementedError(f"tex must be one cube map [1, 6, R, R, 3], got {tuple(tex.shape)}")
    if uv.dim() != 4 or uv.shape[-1] != 3:
        raise NotImplementedError(f"uv must be [B, H, W, 3], got {tuple(uv.shape)}")
    return ops.cubemap_sample(tex[0], uv, filter_mode=filter_mode, boundary_mode=boundary_mode)


def _create_meshgrid(height, width, normalized_coordinates=True, device=None, dtype=None):
    """kornia's `utils.create_meshgrid` as published: [1, H, W, 2], the last axis (x, y); pixel units 0 .. W-1 / 0 .. H-1, or -1 .. 1
    with normalized_coordinates."""
    import torch
    xs = torch.linspace(0, width - 1, width, device=device, dtype=dtype)
    ys = torch.linspace(0, height - 1, height, device=device, dtype=dtype)
    if normalized_coordinates:
        xs = (xs / (width - 1) - 0.5) * 2
        ys = (ys / (height - 1) - 0.5) * 2
    return torch.stack(torch.meshgrid([xs, ys], indexing="ij"), dim=-1).permute(1, 0, 2).unsqueeze(0)


def _module(name: str, doc: str, **attrs):
    mod = types.ModuleType(name)
    mod.__doc__ = doc
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod
    return mod


def _install_rasterizer_packages(installed: list):
    if _missing("diff_gaussian_rasterization"):
        from . import ops
        _module("diff_gaussian_rasterization", "gspl_amd stand-in for diff_gaussian_rasterization (HIP; gspl_amd.ops.GaussianRasterizer)",
                GaussianRasterizationSettings=ops.GaussianRasterizationSettings, GaussianRasterizer=ops.GaussianRasterizer)
        installed.append("diff_gaussian_rasterization")
    if _missing("diff_accel_gaussian_rasterization"):
        from . import ops, optimizers
        _module("diff_accel_gaussian_rasterization",
                "gspl_amd stand-in for diff_accel_gaussian_rasterization (Taming 3DGS; HIP: gspl_amd.ops.AccelGaussianRasterizer, "
                "gspl_amd.optimizers.SparseGaussianAdam)",
                GaussianRasterizationSettings=ops.AccelRasterizationSettings, GaussianRasterizer=ops.AccelGaussianRasterizer,
                SparseGaussianAdam=optimizers.SparseGaussianAdam)
        installed.append("diff_accel_gaussian_rasterization")
    if _missing("diff_surfel_rasterization"):
        from . import ops
        _module("diff_surfel_rasterization",
                "gspl_amd stand-in for diff_surfel_rasterization (2D Gaussian Splatting; HIP: gspl_amd.ops.SurfelGaussianRasterizer)",
                GaussianRasterizationSettings=ops.SurfelRasterizationSettings, GaussianRasterizer=ops.SurfelGaussianRasterizer)
        installed.append("diff_surfel_rasterization")
    if _missing("gsplat"):
        doc = "gspl_amd stand-in for the gsplat fork (HIP ops of gspl_amd.ops under the fork's module paths)"
        pkg = _module("gsplat", doc, spherical_harmonics=_late("spherical_harmonics"))
        pkg.__path__ = []
        pkg.sh = _module("gsplat.sh", doc, spherical_harmonics=_late("spherical_harmonics"))
        pkg.sh_decomposed = _module("gsplat.sh_decomposed", doc, spherical_harmonics_decomposed=_late("spherical_harmonics_decomposed"))
        pkg.rasterize = _module("gsplat.rasterize", doc, rasterize_gaussians=_late("rasterize_gaussians"))
        pkg.project_gaussians = _module("gsplat.project_gaussians", doc, project_gaussians=_late("project_gaussians"))
        pkg.v0_interfaces = _module("gsplat.v0_interfaces", doc, project_gaussians=_late("project_gaussians"),
                                    rasterize_gaussians=_late("rasterize_gaussians"), rasterize_to_pixels=_rasterize_to_pixels_fork)
        cuda = _module("gsplat.cuda", doc)
        cuda.__path__ = []
        pkg.cuda = cuda
        cuda._wrapper = _module("gsplat.cuda._wrapper", doc, fully_fused_projection=_late("fully_fused_projection"),
                                isect_tiles=_late("isect_tiles"), isect_offset_encode=_late("isect_offset_encode"),
                                spherical_harmonics=_late("spherical_harmonics"), rasterize_to_pixels=_rasterize_to_pixels_fork)
        cuda.isect_tiles_tile_based_culling = _module(
            "gsplat.cuda.isect_tiles_tile_based_culling", doc, isect_tiles_tile_based_culling=_isect_tiles_tile_based_culling,
            isect_offset_encode_tile_based_culling=_isect_offset_encode_tile_based_culling)
        pkg.hit_pixel_count = _module("gsplat.hit_pixel_count", doc, hit_pixel_count=_late("hit_pixel_count"))
        pkg.rasterize_to_weights = _module("gsplat.rasterize_to_weights", doc, rasterize_to_weights=_late("rasterize_to_weights"))
        pkg.utils = _module("gsplat.utils", doc, depth_to_normal=_depth_to_normal)
        from . import optimizers
        pkg.optimizers = _module("gsplat.optimizers", doc, SelectiveAdam=optimizers.SelectiveAdam)
        installed.append("gsplat")


def install() -> list:
    """Returns the names of the shim modules that were installed."""
    installed = []
    _install_rasterizer_packages(installed)
    if _missing("simple_knn"):
        from . import ops
        pkg = _module("simple_knn", "gspl_amd stand-in for simple_knn (HIP; see gspl_amd.ops.distCUDA2)",
                      _C=_module("simple_knn._C", None, distCUDA2=ops.distCUDA2))
        pkg.__path__ = []          # a package, so that `from simple_knn._C import ...` resolves through sys.modules
        installed.append("simple_knn._C")
    if _missing("fused_ssim"):
        from . import ops
        _module("fused_ssim", "gspl_amd stand-in for fused_ssim (HIP; see gspl_amd.ops.fused_ssim)", fused_ssim=ops.fused_ssim)
        installed.append("fused_ssim")
    if _missing("nvdiffrast"):
        doc = "gspl_amd stand-in for nvdiffrast.torch: `texture` on cube maps only (HIP; gspl_amd.ops.cubemap_sample)"
        pkg = _module("nvdiffrast", doc)
        pkg.__path__ = []
        pkg.torch = _module("nvdiffrast.torch", doc, texture=_texture)
        installed.append("nvdiffrast.torch")
    if _missing("kornia"):
        doc = "gspl_amd stand-in for kornia.utils: `create_meshgrid` only (plain torch)"
        pkg = _module("kornia", doc)
        pkg.__path__ = []
        pkg.utils = _module("kornia.utils", doc, create_meshgrid=_create_meshgrid)
        installed.append("kornia.utils")
    if _missing("pytorch3d"):
        doc = "gspl_amd stand-in for pytorch3d.ops: `knn_points` only (HIP; gspl_amd.ops.knn_points)"
        pkg = _module("pytorch3d", doc)
        pkg.__path__ = []
        pkg.ops = _module("pytorch3d.ops", doc, knn_points=_late("knn_points"))
        installed.append("pytorch3d.ops")
    if _missing("tinycudann"):
        from . import hashgrid
        _module("tinycudann", "gspl_amd stand-in for tinycudann: `Encoding` with a HashGrid / DenseGrid only (HIP; gspl_amd.ops.hashgrid_encode)",
                Encoding=hashgrid.Encoding)
        installed.append("tinycudann")
    if _missing("fused_bilagrid"):
        _module("fused_bilagrid", "gspl_amd stand-in for fused_bilagrid (HIP; gspl_amd.bilagrid)",
                **{n: _late(n, "bilagrid") for n in ("BilateralGrid", "slice", "total_variation_loss")})
        installed.append("fused_bilagrid")
    return installed

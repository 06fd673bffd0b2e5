"""
gspl_amd.ops — torch.autograd.Function wrappers over the C-ABI, mirroring the operator interfaces the
reference's renderers call (same names, argument meaning and error behaviour):

  gsplat v1 (internal/renderers/gsplat_v1_renderer.py:8-20)
      fully_fused_projection, isect_tiles, isect_offset_encode, rasterize_to_pixels,
      spherical_harmonics, spherical_harmonics_decomposed
  gsplat v0 (internal/renderers/gsplat_renderer.py:2-4, pypreprocess_gsplat_renderer.py:1-2)
      project_gaussians, rasterize_gaussians
  Inria (internal/renderers/vanilla_renderer.py:14)
      GaussianRasterizationSettings, GaussianRasterizer
  2DGS surfels (internal/renderers/vanilla_2dgs_renderer.py:14, `diff_surfel_rasterization`)
      SurfelRasterizationSettings, SurfelGaussianRasterizer
  3DGS-MCMC (internal/density_controllers/mcmc_density_controller.py:13, `gsplat.relocation`; not registered in compat)
      compute_relocation, perturb_means_, mcmc_regularization
  Bilateral grid (internal/output_processors/bilagrid.py, `fused_bilagrid`; the module-level API is gspl_amd.bilagrid)
      bilagrid_slice, bilagrid_tv
  Surface maps (internal/renderers/vanilla_2dgs_renderer.py:146-170, internal/metrics/gs2d_metrics.py, `gsplat.utils.depth_to_normal`)
      depth_to_normal, gsplat_rays, surfel_maps, surface_reg
  Wide feature maps (internal/renderers/feature_3dgs_renderer.py, gsplat_contrastive_feature_renderer.py: `rasterize_gaussians` with
  32 .. 512 channels over a frozen model)
      rasterize_features
  Periodic Vibration Gaussians (internal/models/periodic_vibration_gaussian.py, internal/renderers/periodic_vibration_gaussian_renderer.py,
  internal/model_components/envlight.py: the vibration transform, and `nvdiffrast.torch.texture` on a cube map)
      pvg_motion, cubemap_sample, envlight_blend
  2DGS mesh extraction (internal/utils/gs2d_mesh_utils.py: the per-camera TSDF fusion in torch, `skimage.measure.marching_cubes`)
      tsdf_init, tsdf_table, tsdf_fuse, marching_tetrahedra, marching_tetrahedra_soup, index_soup
  SegAnyGS smoothing and the similarity regulariser's search (internal/segany_splatting.py:262-309, `pytorch3d.ops.knn_points`;
  internal/metrics/appearance_feature_similarity_regularization_metrics.py:70-74; the module-level API is gspl_amd.segany)
      knn_points, knn_graph, KnnGraph, smooth_features
  SWAG's grid encoding (internal/models/swag_model.py:75-78, `tinycudann.Encoding` with otype HashGrid / DenseGrid)
      hashgrid_levels, HashGridLevels, hashgrid_table, hashgrid_encode, hashgrid_forward, hashgrid_backward
  The appearance-embedding route's per-Gaussian MLP (internal/renderers/gsplat_appearance_embedding_renderer.py:50-93, `tcnn: false`)
      appearance_mlp, appearance_mlp_check, appearance_mlp_forward, appearance_mlp_backward
  The 4D-GS route's HexPlane / K-Planes field (internal/model_components/gs4d_hexplane.py: six `F.grid_sample` per level and a product)
      hexplane_layout, HexPlaneLayout, hexplane_pack, hexplane_box, hexplane_encode, hexplane_forward, hexplane_backward
  The SpotLessSplats route (internal/metrics/spotless_metrics.py: the mask MLP behind a bilinear resampling, `robust_mask`, the error
  histogram of `update_running_stats`, the masked L1; the module-level API is gspl_amd.spotless)
      spotless_mask, spotless_error_stats, spotless_masked_l1, and the launches alone: spotless_mask_forward / _backward,
      spotless_masked_l1_forward / _backward
  The SegAnyGS training step behind the renderer (internal/segany_splatting.py:152-260, 317-419: `mask_preprocess` and the loss of
  `forward_with_loss_calculation`; the module-level API is gspl_amd.segany.use_hip_loss)
      segany_mask_stats, segany_pack_membership, segany_pair_labels, segany_correspondence_loss, and the launches alone:
      segany_loss_forward / segany_loss_backward
  The Glossy-Gaussian route's view-dependent opacity (internal/renderers/glossy_renderer.py `get_opacities`,
  internal/models/glossy_gaussian.py `get_view_dep_opacities`: F.normalize + `eval_sh_decomposed` + clamp in torch ops)
      sh_view_opacities, and the launches alone: sh_view_opacities_forward / sh_view_opacities_backward
  The partition-LoD route's per-frame front (internal/renderers/partition_lod_renderer.py:550-625: distances, thresholds, the frustum
  test, and the concatenation of the chosen levels; the module-level API is gspl_amd.lod)
      lod_select, lod_gather
  The Taming-3DGS density controller's scoring (internal/density_controllers/taming_3dgs_density_controller.py: the nine `normalize`
  calls of a view, each a boolean gather and a `torch.median`, the aggregate of `compute_gaussian_score`, and the PIL edge filter of
  `get_edges`; the module-level API is gspl_amd.taming)
      positive_medians, taming_score_accumulate_, find_edges
  The 3D half of the Mip-Splatting route (internal/models/mip_splatting.py: `compute_3d_filter`, a Python loop over every training
  camera with two boolean-index assignments each, and `apply_3d_filter` / `apply_3d_filter_on_scales`, a dozen elementwise launches
  every step; the module-level API is gspl_amd.mip)
      mip_camera_table, mip_filter_3d, mip_apply_3d_filter, and the launches alone: mip_apply_3d_filter_forward / _backward
  The depth-regularisation loss (internal/metrics/inverse_depth_metrics.py `get_inverse_depth_metric`, internal/metrics/depth_metrics.py:
  a normalisation, two masks and a mean over [H, W] in six to ten torch launches each way; the module-level API is gspl_amd.depthreg)
      depth_loss

Host side only: shape checks, buffer allocation through torch's caching allocator, stream hand-off.
All arithmetic happens in libgspl_hip.so; nothing here falls back to PyTorch math.

One module per concern: projection (+ SH colours), binning, compositing, inria (the fused rasterizer), sharded (records and the
three-node step of the Gaussian-sharded renderer), side (radix sort wrappers, distCUDA2, the photometric loss), and one per route; `_common` holds the
streams and the parameter updates in flight, `_args` the argument checks the route ops share, and `_state.STATE` every piece of
mutable run-time state.  This package re-exports all of them under the names the
single-file version had, including the module-level switches (ops.FUSED_INRIA = False still works: they are properties that read
and write STATE).
"""
import sys as _sys
import types as _types

from ._state import STATE, RuntimeState
from ._common import (_SUPPORTED_D, _packed_row_stride, _guarded, _f32c, _rows, _raw_ptr, _grad_or_zeros, _side_stream, colour_stream,
                      join_pending_updates, _await_updates, _take_event, set_deterministic)
from .projection import (_ProjectFn, fully_fused_projection, project_gaussians, _SHFn, spherical_harmonics, spherical_harmonics_decomposed,
                         sh_view_colors, _SHBatchedFn, sh_view_colors_batched)
from .binning import (isect_tiles, isect_offset_encode, _PendingBins, MAX_ISECTS, bin_gaussians_begin, bin_gaussians_end, bin_gaussians, LazyLists,
                      _bin_count_arrived, _bin_finish, _emit)
from .compositing import (_CompositeFn, _composite, rasterize_to_pixels, composite_scores, hit_pixel_count, rasterize_to_weights, rasterize_gaussians)
from .sharded import (unbind_cameras, pack_visible_records, pack_all_records, unpack_visible_records, _PackRecordsFn, _PackAllRecordsFn,
                      _UnpackRecordsFn, _StageCtx, _ShardFrontFn, _ShardExchangeFn, _ShardBackFn, sharded_front, sharded_exchange, sharded_back)
from .inria import (GaussianRasterizationSettings, GaussianRasterizer, _InriaRasterizeFn, _InriaFusedFn, _split_sh, rasterize_inria_accel,
                    AccelRasterizationSettings, AccelGaussianRasterizer)
from .surfel import SurfelRasterizationSettings, SurfelGaussianRasterizer, rasterize_surfels, _SurfelRasterizeFn
from .mcmc import compute_relocation, perturb_means_, mcmc_regularization, mcmc_randn, _MCMCRegFn
from .bilagrid import bilagrid_slice, bilagrid_tv, _SliceFn, _TvFn
from .surface import depth_to_normal, gsplat_rays, surfel_maps, surface_reg, _DepthNormalFn, _SurfelMapsFn, _SurfaceRegFn
from .features import rasterize_features, _FeatureFn
from .pvg import pvg_motion, _PvgMotionFn
from .envlight import cubemap_sample, envlight_blend, _CubemapFn, _BlendFn
from .mesh import tsdf_init, tsdf_table, tsdf_fuse, marching_tetrahedra, marching_tetrahedra_soup, index_soup
from .knn import knn_points, knn_graph, KnnGraph, smooth_features, _SmoothFn
from .hashgrid import hashgrid_levels, HashGridLevels, hashgrid_table, hashgrid_encode, hashgrid_forward, hashgrid_backward, _HashGridFn
from .appearance import appearance_mlp, appearance_mlp_check, appearance_mlp_forward, appearance_mlp_backward, _AppearanceMlpFn
from .hexplane import hexplane_layout, HexPlaneLayout, hexplane_pack, hexplane_box, hexplane_encode, hexplane_forward, hexplane_backward, _HexPlaneFn
from .spotless import (spotless_mask, spotless_mask_forward, spotless_mask_backward, spotless_error_stats, spotless_masked_l1,
                       spotless_masked_l1_forward, spotless_masked_l1_backward, _SpotlessMaskFn, _MaskedL1Fn)
from .segany import (segany_mask_stats, segany_pack_membership, segany_pair_labels, segany_correspondence_loss, segany_loss_forward,
                     segany_loss_backward, SeganyLossState, _SeganyLossFn)
from .glossy import sh_view_opacities, sh_view_opacities_forward, sh_view_opacities_backward, _ShOpacityFn
from .lod import lod_select, lod_gather
from .taming import positive_medians, taming_score_accumulate_, find_edges
from .mip import (mip_camera_table, mip_filter_3d, mip_apply_3d_filter, mip_apply_3d_filter_forward, mip_apply_3d_filter_backward, _MipApplyFn,
                  _MipScalesFn)
from .depthloss import depth_loss, _DepthLossFn
from .side import radix_sort_pairs, radix_sort_keys64, distCUDA2, l1_ssim, fused_ssim, photometric_loss


def _forward(name):
    return property(lambda self: getattr(STATE, name), lambda self, value: setattr(STATE, name, value))


class _OpsPackage(_types.ModuleType):
    """The module-level spellings of the run-time state (read AND write: tests and bench assign to them)."""
    FUSED_INRIA = _forward("fused_inria")
    DEVICE_SIDE_LIST_LENGTH = _forward("device_side_list_length")
    SPECULATIVE_EMIT = _forward("speculative_emit")
    TRACK_HIT_PIXELS = _forward("track_hit_pixels")
    KEEP_LAST_RASTER = _forward("keep_last_raster")
    SIDE_LOW_PRIORITY = _forward("side_low_priority")
    SEGMENTED_BACKWARD = _forward("segmented_backward")
    SPARSE_TAIL = _forward("sparse_tail")
    LAST_RASTER = _forward("last_raster")
    SPECULATION = _forward("speculation")
    PENDING_UPDATES = _forward("pending_updates")
    _LAST_ISECTS = _forward("last_isects")
    _EVENTS = _forward("events")
    _PINNED_WORDS = _forward("pinned_words")
    _PINNED_ENDS = _forward("pinned_ends")


_sys.modules[__name__].__class__ = _OpsPackage

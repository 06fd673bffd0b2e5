"""The Inria API: `GaussianRasterizationSettings`, `GaussianRasterizer` (one fused C call per direction, or the staged calls)."""
from __future__ import annotations

import ctypes
from collections import namedtuple
from typing import NamedTuple

import torch
from torch import Tensor

from .. import _lib as L
from ._state import STATE as S
from ._frame import FrameBlocks
from ._common import (_packed_row_stride, _guarded, _f32c, _grad_or_zeros, _side_stream, colour_stream, _await_updates, _attach_hit_mask,
                      _attach_grad_rows)
from .binning import MAX_ISECTS, bin_gaussians_begin, bin_gaussians_end

# =============================================================================================
# Inria API  (diff_gaussian_rasterization.GaussianRasterizer)
# =============================================================================================
class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: Tensor
    scale_modifier: float
    viewmatrix: Tensor
    projmatrix: Tensor
    sh_degree: int
    campos: Tensor
    prefiltered: bool = False
    debug: bool = False


# `diff_accel_gaussian_rasterization.GaussianRasterizationSettings` (the Taming 3DGS rasterizer package,
# internal/renderers/taming_3dgs_renderer.py:4): the Inria fields and `antialiasing`
AccelRasterizationSettings = namedtuple("AccelRasterizationSettings", GaussianRasterizationSettings._fields + ("antialiasing",),
                                        defaults=(*GaussianRasterizationSettings._field_defaults.values(), False))


def _check_inputs(shs, colors_precomp, *geometry):
    """Upstream's input check, its messages verbatim; `geometry`: (scales, rotations, cov3D_precomp) where a precomputed covariance is
    an alternative to the scale/rotation pair."""
    if (shs is None) == (colors_precomp is None):
        raise Exception("Please provide excatly one of either SHs or precomputed colors!")
    if geometry:
        scales, rotations, cov3D_precomp = geometry
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")


def _split_sh(sh, sh_rest):
    """(sh, sh_rest, n_coeffs) of the rasterizer's colour input: `sh` [N, K, 3] alone, or the reference model's two parameters
    `shs_dc` [N, 1, 3] and `shs_rest` [N, K - 1, 3] (internal/models/vanilla_gaussian.py:266-300), which the kernels then read — and
    whose gradients they write — in place: `get_shs()`'s per-step `torch.cat` (and its backward's two slice copies) never run."""
    if sh is None:
        if sh_rest is not None:
            raise ValueError("shs_rest without shs")
        return None, None, 0
    if sh_rest is None:
        return sh, None, sh.shape[1]
    sh_rest = _f32c(sh_rest)
    if sh.dim() != 3 or sh.shape[1] != 1 or sh_rest.dim() != 3 or sh_rest.shape[0] != sh.shape[0] or sh_rest.shape[2] != 3:
        raise ValueError(f"shs / shs_rest must be [N,1,3] and [N,K-1,3], got {tuple(sh.shape)} and {tuple(sh_rest.shape)}")
    if sh_rest.shape[1] == 0:
        return sh, None, 1
    return sh, sh_rest, 1 + sh_rest.shape[1]


def _forward_inputs(means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, s, sh_rest):
    """The shared opening of the two forwards: every input float32 and contiguous, opacities flat, the SH pair split."""
    means3D = _f32c(means3D)
    sh, colors_precomp, scales, rotations, cov3D_precomp = map(_f32c, (sh, colors_precomp, scales, rotations, cov3D_precomp))
    opac = _f32c(opacities).reshape(-1)
    viewm, projm, campos, bg = _f32c(s.viewmatrix), _f32c(s.projmatrix), _f32c(s.campos), _f32c(s.bg)
    sh, sh_rest, n_coeffs = _split_sh(sh, sh_rest)
    return means3D, sh, sh_rest, n_coeffs, colors_precomp, opac, scales, rotations, cov3D_precomp, viewm, projm, campos, bg


class _InriaRasterizeFn(torch.autograd.Function):
    """The stage-by-stage orchestration (GSPL_FUSED_INRIA=0).  It implements the plain rasterizer only: anti-aliasing and the
    inverse-depth channel (`diff_accel_gaussian_rasterization`, GSPL_INRIA_ANTIALIAS / GSPL_INRIA_INVDEPTH) exist in the fused call
    alone, and `rasterize_inria_accel` raises NotImplementedError for them here."""

    @staticmethod
    @_guarded(1)
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, settings, sh_rest=None):
        s: GaussianRasterizationSettings = settings
        dev = means3D.device
        means3D, sh, sh_rest, n_coeffs, colors_precomp, opac, scales, rotations, cov3D_precomp, viewm, projm, campos, bg = _forward_inputs(
            means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, s, sh_rest)
        N = means3D.shape[0]
        H, W = int(s.image_height), int(s.image_width)
        radii = torch.empty((N,), dtype=torch.int32, device=dev)
        means2d = torch.empty((N, 2), dtype=torch.float32, device=dev)
        depths = torch.empty((N,), dtype=torch.float32, device=dev)
        conics = torch.empty((N, 3), dtype=torch.float32, device=dev)
        colors = torch.empty((N, 3), dtype=torch.float32, device=dev)
        clamped = torch.empty((N, 3), dtype=torch.uint8, device=dev)
        cov3d = torch.empty((N, 6), dtype=torch.float32, device=dev)
        # d colour / d view direction, left by the colour kernel for the backward (which then reads no coefficients for v_means)
        sh_jac = torch.empty((N, 9), dtype=torch.float32, device=dev) if (sh is not None and ctx.needs_input_grad[0]) else None
        tile = 16
        tile_w, tile_h = (W + tile - 1) // tile, (H + tile - 1) // tile
        def preprocess(phases):
            if N > 0:
                if phases & L.GSPL_INRIA_COLOURS:
                    _await_updates(sh, sh_rest)
                L.call("gspl_inria_preprocess_fwd",
                       N, int(s.sh_degree), n_coeffs, L.ptr(means3D), L.ptr(scales), L.ptr(rotations), L.ptr(cov3D_precomp),
                       L.ptr(sh), L.ptr(sh_rest), L.ptr(colors_precomp), L.ptr(viewm), L.ptr(projm), L.ptr(campos), W, H, tile,
                       float(s.tanfovx), float(s.tanfovy), float(s.scale_modifier),
                       L.ptr(radii), L.ptr(means2d), L.ptr(depths), L.ptr(conics), L.ptr(colors), L.ptr(clamped), L.ptr(cov3d),
                       L.ptr(sh_jac) if (phases & L.GSPL_INRIA_COLOURS) else None, phases, L.stream())
        # geometry, then two independent chains: the SH kernel (HBM-bound, one launch) on a side stream, and the count /
        # depth-sort half of the binning (a dozen small latency-bound launches) on the caller's stream; the host meanwhile
        # waits for the one number that sizes the tile sort.
        preprocess(L.GSPL_INRIA_GEOMETRY)
        with _side_stream(dev) as side:
            preprocess(L.GSPL_INRIA_COLOURS)
        pending = bin_gaussians_begin(means2d, depths, radii, H, W, tile, mode=L.GSPL_MODE_INRIA, conics=conics, opacities=opac)
        flat, offsets = bin_gaussians_end(pending)
        side.join()
        n_isects = flat.shape[0]
        out = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        alphas = torch.empty((H, W), dtype=torch.float32, device=dev)
        final_Ts = torch.empty((H, W), dtype=torch.float32, device=dev)
        last_ids = torch.empty((H, W), dtype=torch.int32, device=dev)
        L.call("gspl_composite_fwd", 
            N, n_isects, 3, L.GSPL_MODE_INRIA, L.GSPL_LAYOUT_CHW, L.ptr(means2d), L.ptr(conics), L.ptr(colors), L.ptr(opac),
            L.ptr(bg), W, H, tile, tile_w, tile_h, L.ptr(offsets), L.ptr(flat) if n_isects else None,
            L.ptr(out), L.ptr(alphas), L.ptr(final_Ts), L.ptr(last_ids), None, L.stream())
        ctx.save_for_backward(means3D, scales, rotations, cov3D_precomp, sh, opac, viewm, projm, campos, bg,
                              radii, means2d, conics, colors, clamped, cov3d, offsets, flat, final_Ts, last_ids, sh_jac, sh_rest)
        if S.keep_last_raster:
            S.last_raster = dict(mode=L.GSPL_MODE_INRIA, width=W, height=H, means2d=means2d, conics=conics, opacities=opac,
                               colors=colors, flatten_ids=flat, offsets=offsets, radii=radii, depths=depths, last_ids=last_ids)
        ctx.cfg = (H, W, tile, tile_w, tile_h, int(s.sh_degree), n_coeffs, float(s.tanfovx), float(s.tanfovy),
                   float(s.scale_modifier), colors_precomp is not None, opacities.shape)
        ctx.set_materialize_grads(False)      # the integer `radii` output would otherwise get a zero "gradient" tensor per step
        ctx.mark_non_differentiable(radii)
        ctx.means2D_ref = means2D       # the caller's screen-space tensor: `.has_hit_any_pixels` is attached to it in backward
        return out, radii

    @staticmethod
    @_guarded(0)
    def backward(ctx, v_out, _v_radii):
        (means3D, scales, rotations, cov3D_precomp, sh, opac, viewm, projm, campos, bg,
         radii, means2d, conics, colors, clamped, cov3d, offsets, flat, final_Ts, last_ids, sh_jac, sh_rest) = ctx.saved_tensors
        H, W, tile, tile_w, tile_h, degree, n_coeffs, tanfovx, tanfovy, scale_modifier, has_precomp_colors, opac_shape = ctx.cfg
        N = means3D.shape[0]
        dev = means3D.device
        n_isects = flat.shape[0]
        v_out = _grad_or_zeros(v_out, (3, H, W), dev)
        RS = _packed_row_stride(9)
        packed = torch.zeros((N, RS), dtype=torch.float32, device=dev)       # x y | a b c | opacity | r g b | pad
        if n_isects > 0:
            hit = torch.zeros((N,), dtype=torch.uint8, device=dev) if S.track_hit_pixels else None
            L.call("gspl_composite_bwd_packed",
                N, n_isects, 3, L.GSPL_MODE_INRIA, L.GSPL_LAYOUT_CHW, L.ptr(means2d), L.ptr(conics), L.ptr(colors), L.ptr(opac),
                L.ptr(bg), W, H, tile, tile_w, tile_h, L.ptr(offsets), L.ptr(flat), L.ptr(final_Ts), L.ptr(last_ids),
                L.ptr(v_out), None, L.ptr(packed), RS, 0, L.ptr(hit), L.stream())
            _attach_hit_mask(ctx.means2D_ref, hit)
        v_opac = torch.empty((N,), dtype=torch.float32, device=dev)      # dense copy of the packed column (written below)
        v_means = torch.empty((N, 3), dtype=torch.float32, device=dev)
        v_ndc = torch.empty((N, 3), dtype=torch.float32, device=dev)
        use_cov = cov3D_precomp is not None
        v_scales = None if use_cov else torch.empty((N, 3), dtype=torch.float32, device=dev)
        v_quats = None if use_cov else torch.empty((N, 4), dtype=torch.float32, device=dev)
        v_cov = torch.empty((N, 6), dtype=torch.float32, device=dev) if use_cov else None
        v_sh = None if has_precomp_colors else torch.empty_like(sh)
        v_sh_rest = None if sh_rest is None else torch.empty_like(sh_rest)
        v_cp = torch.empty((N, 3), dtype=torch.float32, device=dev) if has_precomp_colors else None
        if N > 0:
            L.call("gspl_inria_preprocess_bwd", 
                N, degree, n_coeffs, L.ptr(means3D), L.ptr(scales), L.ptr(rotations), L.ptr(cov3d), L.ptr(sh), L.ptr(sh_rest),
                L.ptr(viewm), L.ptr(projm), L.ptr(campos), W, H, tanfovx, tanfovy, scale_modifier,
                L.ptr(radii), L.ptr(clamped), L.ptr(packed), L.ptr(packed, offset_bytes=8), L.ptr(packed, offset_bytes=24), RS,
                L.ptr(v_means), L.ptr(v_scales), L.ptr(v_quats), L.ptr(v_cov), L.ptr(v_sh), L.ptr(v_sh_rest), L.ptr(v_cp), L.ptr(v_ndc),
                L.ptr(packed, offset_bytes=20), L.ptr(v_opac), L.ptr(sh_jac), L.stream())
        # order: means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, settings, sh_rest
        return v_means, v_ndc, v_sh, v_cp, v_opac.reshape(opac_shape), v_scales, v_quats, v_cov, None, v_sh_rest


# ---- the same rasterizer through ONE C-ABI call per direction (gspl_rasterize_inria_fwd/bwd, csrc/fused.hip) -----------------
# The colour stream at the device's lowest priority (a stream from the library; torch cannot create one below the default) or at the
# default priority (the package's torch side stream).  Round 3, 16 rotating cameras, two runs each on one box: no difference for the
# colour kernel alone (1.280 / 1.280 vs 1.292 / 1.273 ms per step), and with the deferred shs_rest update on the same stream the
# default priority is the faster one (1.251 / 1.257 vs 1.266 / 1.264) — and the only two runs with 6-9 ms stalls of single steps had
# the low-priority stream carrying the update.  Default: the default priority.
class _InriaFusedFn(torch.autograd.Function):
    @staticmethod
    @_guarded(1)
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, settings, sh_rest=None, raw_params=False,
                antialias=False, invdepth=False):
        """raw_params: `opacities`, `scales`, `rotations` are the model's RAW parameters; sigmoid / exp / normalize run inside the preprocess
        kernels (GSPL_INRIA_RAW_PARAMS) and the backward returns the raw parameters' gradients.
        antialias: the composited opacity is opacity * sqrt(max(2.5e-5, det0 / det1)) (GSPL_INRIA_ANTIALIAS).
        invdepth: the output is [4,H,W], colour and the composited inverse view-space depth (background 0; GSPL_INRIA_INVDEPTH)."""
        s: GaussianRasterizationSettings = settings
        dev = means3D.device
        means3D, sh, sh_rest, n_coeffs, colors_precomp, opac, scales, rotations, cov3D_precomp, viewm, projm, campos, bg = _forward_inputs(
            means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, s, sh_rest)
        N = means3D.shape[0]
        H, W = int(s.image_height), int(s.image_width)
        D = 4 if invdepth else 3
        if invdepth:      # the inverse-depth channel's background is 0
            bg = torch.cat([bg.reshape(-1)[:3], bg.new_zeros(1)])
        out = torch.empty((D, H, W), dtype=torch.float32, device=dev)
        radii = torch.empty((N,), dtype=torch.int32, device=dev)
        tile_w, tile_h = (W + 15) // 16, (H + 15) // 16
        key = (dev.index, tile_w, tile_h)
        hint = min(S.capacity.hint(key, N), MAX_ISECTS) if S.speculative_emit else 0      # (0: no history for this device and tile grid yet)
        state = L.InriaState()
        will_backward = any(ctx.needs_input_grad)
        state.flags = (L.GSPL_INRIA_RAW_PARAMS if raw_params else 0) | ((L.GSPL_INRIA_FORCE_SEGMENTS if S.segmented_backward == "always" else 0)
                       if (S.segmented_backward and will_backward) else L.GSPL_INRIA_NO_SEGMENTS)      # (only a frame that can have a backward)
        state.flags |= (L.GSPL_INRIA_ANTIALIAS if antialias else 0) | (L.GSPL_INRIA_INVDEPTH if invdepth else 0)
        if will_backward:
            state.flags |= L.GSPL_INRIA_WILL_BACKWARD      # the forward's compositing kernel clears the backward's packed rows (no fill command there)
        side = _side_stream(dev)
        with torch.cuda.device(dev):
            side_handle = None
            low = False
            raw = None
            if side.enabled:
                # the colour stream (default priority; GSPL_SIDE_LOW_PRIORITY=1: the library's lowest-priority stream, on which the
                # colour kernel yields to the key pass and the depth sort it runs next to)
                raw, _ = colour_stream(dev)
                low = _side_stream._low.get((dev.type, dev.index), False)
                side_handle = ctypes.c_void_p(raw)
            # coefficient updates still in flight (FusedAdam(deferred=...)): on the colour stream itself stream order covers them
            _await_updates(sh, sh_rest, on_raw_stream=raw)
            # geometry parameters are read on the CALLER's stream (also in place with raw_params): an update of theirs in flight on
            # the colour stream has to be over first (FusedAdam(deferred=("scales", ...)): "kernels of this package wait by themselves")
            _await_updates(means3D, scales, rotations, opac)
            with FrameBlocks(dev) as frame:
                L.call("gspl_rasterize_inria_fwd", N, int(s.sh_degree), n_coeffs, L.ptr(means3D), L.ptr(scales), L.ptr(rotations),
                       L.ptr(cov3D_precomp), L.ptr(sh), L.ptr(sh_rest), L.ptr(colors_precomp), L.ptr(opac), L.ptr(viewm), L.ptr(projm), L.ptr(campos), L.ptr(bg),
                       W, H, float(s.tanfovx), float(s.tanfovy), float(s.scale_modifier), frame.callback, None, hint,
                       L.ptr(out), L.ptr(radii), ctypes.byref(state), L.stream(), side_handle)
        if side.enabled and not low:
            # blocks the colour kernel used on the side stream are freed by the caller's stream: tell the allocator
            # (the library's own low-priority stream is joined inside the call: stream order on the caller's stream covers it)
            frame.kept[L.GSPL_BUF_GEOMETRY].record_stream(side.stream)
        S.last_isects[key] = int(state.n_isects)
        S.capacity.observe(key, N, int(state.n_isects))
        S.speculation["frames"] += 1
        if hint == 0:
            S.speculation["cold"] += 1
        elif int(state.n_isects) > hint:
            S.speculation["misses"] += 1
        ctx.cfg = (H, W, int(s.sh_degree), n_coeffs, float(s.tanfovx), float(s.tanfovy), float(s.scale_modifier), colors_precomp is not None,
                   cov3D_precomp is not None, opacities.shape, D)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(radii)
        ctx.means2D_ref = means2D
        if S.keep_last_raster:
            nI = int(state.n_isects)
            S.last_raster = dict(mode=L.GSPL_MODE_INRIA, width=W, height=H, means2d=frame.view(state.means2d, (N, 2), torch.float32),
                               conics=frame.view(state.conics, (N, 3), torch.float32),
                               opacities=(frame.view(state.opacities, (N,), torch.float32) if (raw_params or antialias) else opac),
                               colors=frame.view(state.colors, (N, D), torch.float32),
                               flatten_ids=(frame.view(state.flatten_ids, (nI,), torch.int32) if state.flatten_ids else torch.empty(0, dtype=torch.int32, device=dev)),
                               offsets=frame.view(state.offsets, (tile_w * tile_h,), torch.int32), radii=radii,
                               depths=frame.view(state.depths, (N,), torch.float32),
                               last_ids=frame.view(state.last_ids, (H, W), torch.int32),
                               # segmented backward: the word in which the backward counts the segments it published (beyond each tile's
                               # first; 0 after a backward: every walk was short; None: no checkpoints were taken)
                               segment_count=(frame.view(state.seg_words, (1,), torch.int32) if state.seg_ckpt else None))
        # The frame's device blocks (projected splats, tile lists, per-pixel state, checkpoints, packed rows) are SAVED TENSORS of the node:
        # autograd frees them when the graph is released — right after the backward, or, with `retain_graph=True`, when the graph dies —
        # and a second backward through a released graph raises autograd's own error, as with the Inria op this replaces.
        ctx.save_for_backward(means3D, scales, rotations, sh, opac, viewm, projm, campos, bg, radii, sh_rest, *frame.saved())
        ctx.state, ctx.frame, ctx.backwards_run = state, frame, 0
        return out, radii

    @staticmethod
    @_guarded(0)
    def backward(ctx, v_out, _v_radii):
        means3D, scales, rotations, sh, opac, viewm, projm, campos, bg, radii, sh_rest, *saved_blocks = ctx.saved_tensors      # (a released graph raises here)
        blocks = ctx.frame.unpack(saved_blocks)
        H, W, degree, n_coeffs, tanfovx, tanfovy, scale_modifier, has_precomp_colors, use_cov, opac_shape, D = ctx.cfg
        prow = 6 + D      # the packed row: x y | a b c | opacity | colour (| 1/z)
        N = means3D.shape[0]
        dev = means3D.device
        ctx.backwards_run += 1
        if ctx.backwards_run > 1 and ctx.state.seg_ckpt:
            # retain_graph: the segmented backward counts the segments it publishes in two words the FORWARD kernel cleared — clear them again
            blocks.view(ctx.state.seg_words, (2,), torch.int32).zero_()
        v_out = _grad_or_zeros(v_out, (D, H, W), dev)
        E = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        if ctx.state.flags & L.GSPL_INRIA_PACKED_READY:      # the block the forward's compositing kernel cleared: the C side clears nothing
            packed = blocks.view(ctx.frame.addresses[L.GSPL_BUF_PACKED], (N, prow), torch.float32)
            if ctx.backwards_run > 1:
                packed.zero_()      # retain_graph: the rows hold the first backward's sums
        else:
            packed = E(N, prow)
        hit = torch.empty((N,), dtype=torch.uint8, device=dev) if S.track_hit_pixels else None
        # the density controller's statistics of THIS frame (density.request_stats_in_backward: the request names the radii this
        # forward returned): the preprocess-backward kernel applies them, once
        stats = S.backward_stats
        if stats is not None and N > 0 and stats.radii_ptr == radii.data_ptr() and stats.n == N and not stats.applied:
            S.backward_stats = None
            ctx.state.stats_accum, ctx.state.stats_denom = stats.accum.data_ptr(), stats.denom.data_ptr()
            ctx.state.stats_max_radii = stats.max_radii.data_ptr() if stats.max_radii is not None else None
        else:
            stats = None
        # An optimizer built with fuse_into_backward=True that owns EVERY parameter differentiated here: the kernels that end the
        # backward apply its update themselves (gspl_rasterize_inria_bwd_adam) and no parameter gradient is written or returned
        # (not for a frame with anti-aliasing or inverse depth: gspl_rasterize_inria_bwd_adam refuses them, the optimizer then steps itself)
        extended = bool(ctx.state.flags & (L.GSPL_INRIA_ANTIALIAS | L.GSPL_INRIA_INVDEPTH))
        plan = None
        if S.backward_optimizers and N > 0 and not use_cov and not has_precomp_colors and not extended:
            need = ctx.needs_input_grad
            if need[0] and need[2] and need[4] and need[5] and need[6] and (sh_rest is None or need[9]):
                from ..optimizers import claim_backward_update
                plan = claim_backward_update(dict(means=means3D, scales=scales, rotations=rotations, opacities=opac, shs=sh, shs_rest=sh_rest))
        if plan is not None:
            scratch, v_ndc = E(N, 3), E(N, 3)
        else:
            v_means, v_ndc, v_opac = E(N, 3), E(N, 3), E(N)
            v_scales = None if use_cov else E(N, 3)
            v_quats = None if use_cov else E(N, 4)
            v_cov = E(N, 6) if use_cov else None
            v_sh = None if has_precomp_colors else torch.empty_like(sh)
            v_sh_rest = None if sh_rest is None else torch.empty_like(sh_rest)
            v_cp = E(N, 3) if has_precomp_colors else None
        # the sparse tail (STATE.sparse_tail): the C side clears the gradient arrays itself and says which rows it then wrote
        grad_rows = torch.empty((N,), dtype=torch.uint8, device=dev) if (plan is None and S.sparse_tail and N > 0) else None
        if N > 0:
            try:
                with torch.cuda.device(dev):
                    if plan is not None:
                        L.call("gspl_rasterize_inria_bwd_adam", degree, n_coeffs, L.ptr(means3D), L.ptr(scales), L.ptr(rotations), L.ptr(sh),
                               L.ptr(sh_rest), L.ptr(opac), L.ptr(viewm), L.ptr(projm), L.ptr(campos), L.ptr(bg), tanfovx, tanfovy, scale_modifier,
                               L.ptr(radii), ctypes.byref(ctx.state), L.ptr(v_out), L.ptr(packed), L.ptr(hit), L.ptr(scratch), L.ptr(v_ndc),
                               ctypes.byref(plan), L.stream())
                    elif grad_rows is not None:
                        L.call("gspl_rasterize_inria_bwd_sparse", degree, n_coeffs, L.ptr(means3D), L.ptr(scales), L.ptr(rotations), L.ptr(sh),
                               L.ptr(sh_rest), L.ptr(opac), L.ptr(viewm), L.ptr(projm), L.ptr(campos), L.ptr(bg), tanfovx, tanfovy, scale_modifier,
                               L.ptr(radii), ctypes.byref(ctx.state), L.ptr(v_out), L.ptr(packed), L.ptr(hit), L.ptr(v_means), L.ptr(v_ndc), L.ptr(v_sh),
                               L.ptr(v_sh_rest), L.ptr(v_cp), L.ptr(v_opac), L.ptr(v_scales), L.ptr(v_quats), L.ptr(v_cov), L.ptr(grad_rows), L.stream())
                    else:
                        L.call("gspl_rasterize_inria_bwd", degree, n_coeffs, L.ptr(means3D), L.ptr(scales), L.ptr(rotations), L.ptr(sh), L.ptr(sh_rest),
                               L.ptr(opac), L.ptr(viewm), L.ptr(projm), L.ptr(campos), L.ptr(bg), tanfovx, tanfovy, scale_modifier, L.ptr(radii),
                               ctypes.byref(ctx.state), L.ptr(v_out), L.ptr(packed), L.ptr(hit), L.ptr(v_means), L.ptr(v_ndc), L.ptr(v_sh), L.ptr(v_sh_rest),
                               L.ptr(v_cp), L.ptr(v_opac), L.ptr(v_scales), L.ptr(v_quats), L.ptr(v_cov), L.stream())
            except Exception:
                _poison(ctx, stats)
                raise
            if stats is not None:
                stats.applied = True
                ctx.state.stats_accum = ctx.state.stats_denom = ctx.state.stats_max_radii = None
            _attach_hit_mask(ctx.means2D_ref, hit)
            if plan is not None:
                return None, v_ndc, None, None, None, None, None, None, None, None, None, None, None
            if S.keep_last_raster and S.last_raster is not None:
                # introspection (tests): the compositing backward's own per-splat rows, x y | a b c | opacity | r g b
                S.last_raster["packed_grads"] = packed
                S.last_raster["grad_rows"] = grad_rows
            if grad_rows is not None:
                _attach_grad_rows(grad_rows, v_means, v_sh, v_cp, v_opac, v_scales, v_quats, v_cov, v_sh_rest)
        else:
            for t in (v_means, v_ndc, v_opac):
                t.zero_()
        return v_means, v_ndc, v_sh, v_cp, v_opac.reshape(opac_shape), v_scales, v_quats, v_cov, None, v_sh_rest, None, None, None


def _poison(ctx, stats):
    """A fused backward call that raised: the statistics pointers leave the frame's state — a retried backward must not hand
    them to the kernel again — and the request counts as consumed: part of the launch sequence may have run and added the frame's
    statistics already, so the controller's fall-back launch must not add them a second time."""
    ctx.state.stats_accum = ctx.state.stats_denom = ctx.state.stats_max_radii = None
    if stats is not None:
        stats.applied = True


def _rasterize(settings, means3D, means2D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp, shs_rest, raw_parameters,
               antialiasing=False, inverse_depth=False):
    """The one way into the two autograd functions, for `GaussianRasterizer` and `rasterize_inria_accel`: checks the inputs, drops an
    empty `shs_rest`, and makes one C-ABI call per direction (csrc/fused.hip) unless GSPL_FUSED_INRIA=0 selects the stage-by-stage
    orchestration.  The radii of a fused call say so: its backward can take the frame's densification statistics along (density.py)."""
    if isinstance(shs, (tuple, list)):
        shs, shs_rest = shs
    _check_inputs(shs, colors_precomp, scales, rotations, cov3D_precomp)
    if not S.fused_inria and (antialiasing or inverse_depth):
        raise NotImplementedError("anti-aliasing and inverse depth exist in the fused Inria call only (GSPL_FUSED_INRIA=0 selects the staged one)")
    if shs_rest is not None and shs_rest.shape[1] == 0:
        shs_rest = None
    if raw_parameters and cov3D_precomp is not None:
        raise Exception("raw_parameters needs the scale/rotation pair")
    if S.fused_inria:
        out = _InriaFusedFn.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, settings, shs_rest,
                                  bool(raw_parameters), bool(antialiasing), bool(inverse_depth))
        out[1]._gspl_fused_inria = True
        return out
    if raw_parameters:      # the stage-by-stage orchestration takes activated values: the same three activations through torch
        opacities, scales, rotations = torch.sigmoid(opacities), torch.exp(scales), torch.nn.functional.normalize(rotations)
    return _InriaRasterizeFn.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, settings, shs_rest)


class GaussianRasterizer(torch.nn.Module):
    """Drop-in for `diff_gaussian_rasterization.GaussianRasterizer` as the reference uses it
    (internal/renderers/vanilla_renderer.py:79,111-120): returns (color [3,H,W], radii [N] i32);
    `means2D.grad` receives the screen-space gradient in the Inria (NDC-scaled) units."""

    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, shs_rest=None, raw_parameters: bool = False):
        """`shs_rest` (extension; also accepted as `shs=(shs_dc, shs_rest)`): the model's two SH parameters as they are stored.
        `raw_parameters` (extension): `opacities`, `scales`, `rotations` are the model's RAW parameters — logits, log-scales,
        unnormalised quaternions — and the activations of the reference's model (sigmoid / exp / F.normalize,
        internal/models/vanilla_gaussian.py:345-358) run inside the preprocess kernels, forward and backward, instead of as ten torch
        launches and a reduction per step around the call."""
        return _rasterize(self.raster_settings, means3D, means2D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp, shs_rest,
                          raw_parameters)


def rasterize_inria_accel(settings: GaussianRasterizationSettings, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                          rotations=None, cov3D_precomp=None, shs_rest=None, raw_parameters: bool = False, antialiasing: bool = False,
                          inverse_depth: bool = True):
    """The fused Inria call with the two switches of `diff_accel_gaussian_rasterization` (Taming 3DGS): `antialiasing` (the Mip-Splatting
    2D filter, GSPL_INRIA_ANTIALIAS) and `inverse_depth` (a 4th composited channel 1 / z, GSPL_INRIA_INVDEPTH).  Returns (color [3,H,W],
    radii [N] i32, inverse depth [1,H,W] or None); the two images are views of one [4,H,W] output.  Arguments as `GaussianRasterizer`.
    There is no stage-by-stage form of these switches: with GSPL_FUSED_INRIA=0 they raise NotImplementedError."""
    out, radii = _rasterize(settings, means3D, means2D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp, shs_rest,
                            raw_parameters, antialiasing, inverse_depth)
    if inverse_depth:
        return out[:3], radii, out[3:]
    return out, radii, None


class AccelGaussianRasterizer(torch.nn.Module):
    """Drop-in for `diff_accel_gaussian_rasterization.GaussianRasterizer` as the reference calls it
    (internal/renderers/taming_3dgs_renderer.py:66-96): returns (color [3,H,W], radii [N] i32, inverse depth [1,H,W]).  `dc` [N,1,3] and
    `shs` [N,K-1,3] are the two SH parameters (read in place as `shs` / `shs_rest`); `means2D.grad` receives the same NDC-scaled
    screen-space gradient as `GaussianRasterizer`'s.  Runs the fused call with GSPL_INRIA_INVDEPTH (and GSPL_INRIA_ANTIALIAS when the
    settings ask for it)."""

    def __init__(self, raster_settings: AccelRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward(self, means3D, means2D, dc=None, shs=None, colors_precomp=None, opacities=None, scales=None, rotations=None, cov3D_precomp=None,
                raw_parameters: bool = False):
        if colors_precomp is not None:
            sh, sh_rest = None, None
        elif dc is None:
            sh, sh_rest = shs, None
        else:
            sh, sh_rest = dc, shs
        _check_inputs(sh, colors_precomp)
        return rasterize_inria_accel(self.raster_settings, means3D, means2D, opacities, sh, colors_precomp, scales, rotations, cov3D_precomp,
                                     shs_rest=sh_rest, raw_parameters=raw_parameters,
                                     antialiasing=bool(getattr(self.raster_settings, "antialiasing", False)), inverse_depth=True)

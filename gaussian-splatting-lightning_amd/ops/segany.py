"""The SegAnyGS (SAGA) training step behind the renderer (internal/segany_splatting.py:152-260, 317-419; include/gspl_hip.h section 24,
csrc/segany.hip).

  segany_mask_stats(masks, order=None) -> (area [N] int32, cover [H, W] int32, mean_size [H, W] f32): the masks read once, a byte per
      entry; no float copy and no permuted copy of them is made.
  segany_pack_membership(masks, order, pixel_index) -> bits [S, ceil(N / 64)] int64: bit i of a row = the i-th mask in the order of
      descending scale holds that sampled pixel.
  segany_pair_labels(bits, scale_index, upper, n_masks=None) -> (labels [S, S] uint16, counts [3] int32): bit n of a label =
      gt_corrs[n, h, j]; both triangles are written.
  segany_correspondence_loss(rendered, mask_hw, pixel_index, gates, labels, counts, a, rand) -> (loss, cosine_pos, cosine_neg),
      differentiable in `rendered` and `gates`; `segany_loss_forward` / `segany_loss_backward` are the launches alone.

GPU only, float32; no fallback.  The reference's arithmetic is torch code: the fp64 oracle tests/segany_loss_oracle.py is pinned to it
through tests/golden/ref_segany_loss.npz, and the kernels to the oracle."""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from .. import _lib as L
from . import _args as A, _frame
from ._common import _guarded

MAX_S = 4096
MAX_MASKS = 1024
MAX_SCALES = 16
MAX_C = 64
MAX_DIM = 16384


def _masks(who: str, masks) -> Tuple[Tensor, int, int, int]:
    m = A.gpu_tensor(who, "masks", masks, torch.bool, torch.uint8).detach().contiguous()
    if m.dim() != 3:
        raise ValueError(f"{who}: masks must be [N, H, W], got {tuple(m.shape)}")
    N, H, W = m.shape
    if not 1 <= N <= MAX_MASKS:
        raise NotImplementedError(f"{who}: 1 .. {MAX_MASKS} masks are built, got {N}")
    if min(H, W) < 1 or max(H, W) > MAX_DIM:
        raise NotImplementedError(f"{who}: H and W must be 1 .. {MAX_DIM}, got {(H, W)}")
    return m.view(torch.uint8), N, H, W


def _order(who: str, order, N: int, like: Tensor) -> Tensor:
    o = A.gpu_tensor(who, "order", order, torch.int32, torch.int64, like=like).detach().contiguous()
    if tuple(o.shape) != (N,):
        raise ValueError(f"{who}: order must be [{N}], got {tuple(o.shape)}")
    return o.to(torch.int32)


def _pixel_index(who: str, pixel_index, like: Tensor) -> Tensor:
    p = A.gpu_tensor(who, "pixel_index", pixel_index, torch.int32, torch.int64, like=like).detach().contiguous()
    if p.dim() != 1 or not 1 <= p.numel() <= MAX_S:
        raise NotImplementedError(f"{who}: pixel_index must be [S] with 1 <= S <= {MAX_S}, got {tuple(p.shape)}")
    return p.to(torch.int32)


def _block(nbytes: int, device) -> Tensor:
    """A scratch block through the library's allocation hook (256-byte aligned, as torch's blocks are; tests put guard bands around it)."""
    return _frame.allocate(max(int(nbytes), 1), device, 0)


@_guarded(0)
def segany_mask_stats(masks: Tensor, order: Optional[Tensor] = None):
    """masks [N, H, W] bool or uint8 on the GPU -> (area [N] int32: pixels per mask; cover [H, W] int32: masks per pixel;
    mean_size [H, W] float32 = (sum_i mask_i(p) area_i) / (cover + 1e-9), the numerator exact in 64-bit integers and rounded once —
    the reference's `per_pixel_mean_mask_size`).  The three are independent of the masks' order; `order` is accepted (and checked)
    so that the call reads like the reference's sorted one.  Scratch: 8 bytes per pixel and 64 masks."""
    who = "segany_mask_stats"
    m, N, H, W = _masks(who, masks)
    if order is not None:
        _order(who, order, N, m)
    area = torch.zeros((N,), dtype=torch.int32, device=m.device)
    cover = torch.empty((H, W), dtype=torch.int32, device=m.device)
    mean_size = torch.empty((H, W), dtype=torch.float32, device=m.device)
    packed = _block(((N + 63) // 64) * H * W * 8, m.device)
    L.call("gspl_segany_mask_stats", N, H, W, L.ptr(m), L.ptr(area), L.ptr(cover), L.ptr(mean_size), L.ptr(packed), L.stream())
    return area, cover, mean_size


@_guarded(0)
def segany_pack_membership(masks: Tensor, order: Tensor, pixel_index: Tensor) -> Tensor:
    """masks [N, H, W], order [N] (the permutation that sorts the masks' scales descending), pixel_index [S] flat indices into H W ->
    bits [S, ceil(N / 64)] int64: bit i of word w = mask order[64 w + i] holds the pixel.  S x N bytes of the masks are read."""
    who = "segany_pack_membership"
    m, N, H, W = _masks(who, masks)
    o, p = _order(who, order, N, m), _pixel_index(who, pixel_index, m)
    bits = torch.empty((p.numel(), (N + 63) // 64), dtype=torch.int64, device=m.device)
    L.call("gspl_segany_pack_membership", N, H, W, p.numel(), L.ptr(m), L.ptr(o), L.ptr(p), L.ptr(bits), L.stream())
    return bits


@_guarded(0)
def segany_pair_labels(bits: Tensor, scale_index: Tensor, upper: Tensor, n_masks: Optional[int] = None):
    """bits [S, NW] int64 (segany_pack_membership), scale_index [Ns] (the reference's `sampled_scale_index`, entry 0 holding -1),
    upper [Ns] bool or uint8 (the `upper_bound` flag of each sampled scale) -> (labels [S, S] uint16, counts [3] int32).
    Bit n of labels[h, j] = gt_corrs[n, h, j]; the matrix is symmetric and both triangles are written.  counts, over the full matrix
    with the diagonal: pairs labelled 1 at no scale, at every scale, and the rest.  Integers throughout: exact."""
    who = "segany_pair_labels"
    b = A.gpu_tensor(who, "bits", bits, torch.int64).detach().contiguous()
    if b.dim() != 2 or not 1 <= b.shape[0] <= MAX_S or not 1 <= b.shape[1] <= MAX_MASKS // 64:
        raise NotImplementedError(f"{who}: bits must be [S <= {MAX_S}, NW <= {MAX_MASKS // 64}], got {tuple(b.shape)}")
    S, NW = b.shape
    N = 64 * NW if n_masks is None else int(n_masks)
    if (N + 63) // 64 != NW:
        raise ValueError(f"{who}: {N} masks need {(N + 63) // 64} words, bits has {NW}")
    si = A.gpu_tensor(who, "scale_index", scale_index, torch.int32, torch.int64, like=b).detach().contiguous().to(torch.int32)
    up = A.gpu_tensor(who, "upper", upper, torch.bool, torch.uint8, like=b).detach().contiguous().view(torch.uint8)
    Ns = si.numel()
    if si.dim() != 1 or up.shape != si.shape or not 1 <= Ns <= MAX_SCALES:
        raise NotImplementedError(f"{who}: scale_index and upper must be [Ns] with 1 <= Ns <= {MAX_SCALES}, got {tuple(si.shape)}, {tuple(up.shape)}")
    labels = torch.empty((S, S), dtype=torch.uint16, device=b.device)
    counts = torch.zeros((3,), dtype=torch.int32, device=b.device)
    head = _block(Ns * S * 4, b.device)
    L.call("gspl_segany_pair_labels", S, N, Ns, L.ptr(b), L.ptr(si), L.ptr(up), L.ptr(head), L.ptr(labels), L.ptr(counts), L.stream())
    return labels, counts


class SeganyLossState(NamedTuple):
    """What the forward leaves for the backward and for tests."""
    out: Tensor             # [3] loss, cosine_pos, cosine_neg
    F: Tensor               # [S, C] the sampled features
    selected: Tensor        # [S, S] uint8: bit 0 in M+, bit 1 in M- (h < j; zero elsewhere)
    sel_counts: Tensor      # [2] int32 |M+|, |M-|
    weight: Optional[Tensor]


def _loss_inputs(who, rendered, mask_hw, pixel_index, gates, labels, counts, a, rand):
    r = A.gpu_tensor(who, "rendered", rendered, torch.float32).detach().contiguous()
    if r.dim() != 3:
        raise ValueError(f"{who}: rendered must be [C, H, W], got {tuple(r.shape)}")
    C, Hr, Wr = r.shape
    if C % 4 or not 4 <= C <= MAX_C:
        raise NotImplementedError(f"{who}: C must be a multiple of 4, 4 .. {MAX_C}, got {C}")
    mh, mw = int(mask_hw[0]), int(mask_hw[1])
    if min(Hr, Wr, mh, mw) < 1 or max(Hr, Wr, mh, mw) > MAX_DIM:
        raise NotImplementedError(f"{who}: every image dimension must be 1 .. {MAX_DIM}, got {(Hr, Wr)} and {(mh, mw)}")
    p = _pixel_index(who, pixel_index, r)
    S = p.numel()
    g = A.gpu_tensor(who, "gates", gates, torch.float32, like=r).detach().contiguous()
    if g.dim() != 2 or g.shape[1] != C or not 1 <= g.shape[0] <= MAX_SCALES:
        raise NotImplementedError(f"{who}: gates must be [Ns <= {MAX_SCALES}, {C}], got {tuple(g.shape)}")
    Ns = g.shape[0]
    lab = A.gpu_tensor(who, "labels", labels, torch.uint16, like=r).detach().contiguous()
    cnt = A.gpu_tensor(who, "counts", counts, torch.int32, like=r).detach().contiguous()
    av = A.gpu_tensor(who, "a", a, torch.float32, like=r).detach().contiguous()
    if tuple(lab.shape) != (S, S) or tuple(cnt.shape) != (3,) or tuple(av.shape) != (S,):
        raise ValueError(f"{who}: labels must be [{S}, {S}], counts [3], a [{S}]; got {tuple(lab.shape)}, {tuple(cnt.shape)}, {tuple(av.shape)}")
    rnd = None
    if rand is not None:
        rnd = A.gpu_tensor(who, "rand", rand, torch.float32, like=r).detach().contiguous()
        if tuple(rnd.shape) != (S, S):
            raise ValueError(f"{who}: rand must be [{S}, {S}], got {tuple(rnd.shape)}")
    return r, (S, C, Ns, Hr, Wr, mh, mw), p, g, lab, cnt, av, rnd


def _workspace(S, C, Ns, device):
    nbytes = L.lib().gspl_segany_loss_workspace_bytes(S, C, Ns)
    return _block(nbytes, device), nbytes


@_guarded(0)
def segany_loss_forward(rendered: Tensor, mask_hw, pixel_index: Tensor, gates: Tensor, labels: Tensor, counts: Tensor, a: Tensor,
                        rand: Tensor, with_weight: bool = False) -> SeganyLossState:
    """The five forward launches alone, outside autograd -> SeganyLossState.  `with_weight`: also the [S, S] matrix of the in-kernel
    pair weight (for tests; the loss never reads a weight matrix)."""
    who = "segany_loss_forward"
    r, shape, p, g, lab, cnt, av, rnd = _loss_inputs(who, rendered, mask_hw, pixel_index, gates, labels, counts, a, rand)
    S, C, Ns = shape[:3]
    dev = r.device
    F = torch.empty((S, C), dtype=torch.float32, device=dev)
    out = torch.empty((3,), dtype=torch.float32, device=dev)
    sel_counts = torch.empty((2,), dtype=torch.int32, device=dev)
    selected = torch.zeros((S, S), dtype=torch.uint8, device=dev)
    weight = torch.empty((S, S), dtype=torch.float32, device=dev) if with_weight else None
    workspace, nbytes = _workspace(S, C, Ns, dev)
    L.call("gspl_segany_loss_fwd", *shape, L.ptr(r), L.ptr(p), L.ptr(g), L.ptr(lab), L.ptr(cnt), L.ptr(av), L.ptr(rnd), L.ptr(F), L.ptr(out),
           L.ptr(sel_counts), L.ptr(selected), L.ptr(weight), L.ptr(workspace), nbytes, L.stream())
    return SeganyLossState(out, F, selected, sel_counts, weight)


@_guarded(3)
def segany_loss_backward(state: SeganyLossState, rendered_shape, mask_hw, pixel_index: Tensor, gates: Tensor, labels: Tensor, a: Tensor,
                         grad_out: Tensor, need_rendered: bool = True):
    """The backward launches alone: grad_out [1] on the device -> (v_F [S, C], v_gates [Ns, C], v_rendered [C, Hr, Wr] or None).
    v_F and v_gates have the same bits on every run; v_rendered is scattered with float atomics (samples share texels)."""
    who = "segany_loss_backward"
    F = state.F
    S, C = F.shape
    Hr, Wr = int(rendered_shape[-2]), int(rendered_shape[-1])
    mh, mw = int(mask_hw[0]), int(mask_hw[1])
    p = _pixel_index(who, pixel_index, F)
    g = A.gpu_tensor(who, "gates", gates, torch.float32, like=F).detach().contiguous()
    lab = A.gpu_tensor(who, "labels", labels, torch.uint16, like=F).detach().contiguous()
    av = A.gpu_tensor(who, "a", a, torch.float32, like=F).detach().contiguous()
    go = A.gpu_tensor(who, "grad_out", grad_out, torch.float32, like=F).detach().contiguous()
    Ns = g.shape[0]
    if (p.numel() != S or g.dim() != 2 or g.shape[1] != C or tuple(lab.shape) != (S, S) or tuple(av.shape) != (S,) or go.numel() != 1
            or tuple(state.selected.shape) != (S, S) or tuple(state.sel_counts.shape) != (2,)):
        raise ValueError(f"{who}: the arguments do not have the shapes of the forward's (S = {S}, C = {C})")
    dev = F.device
    v_F = torch.empty((S, C), dtype=torch.float32, device=dev)
    v_gates = torch.empty((Ns, C), dtype=torch.float32, device=dev)
    v_rendered = torch.zeros((C, Hr, Wr), dtype=torch.float32, device=dev) if need_rendered else None
    workspace, nbytes = _workspace(S, C, Ns, dev)
    L.call("gspl_segany_loss_bwd", S, C, Ns, Hr, Wr, mh, mw, L.ptr(p), L.ptr(g), L.ptr(lab), L.ptr(av), L.ptr(state.selected, torch.uint8),
           L.ptr(state.sel_counts, torch.int32), L.ptr(F, torch.float32), L.ptr(go), L.ptr(v_F), L.ptr(v_gates), L.ptr(v_rendered),
           L.ptr(workspace), nbytes, L.stream())
    return v_F, v_gates, v_rendered


class _SeganyLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rendered, gates, mask_hw, pixel_index, labels, counts, a, rand):
        state = segany_loss_forward(rendered, mask_hw, pixel_index, gates, labels, counts, a, rand)
        ctx.save_for_backward(state.F, state.selected, state.sel_counts, pixel_index, gates.detach().contiguous(), labels, a)
        ctx.mask_hw, ctx.rendered_shape, ctx.gates_shape = mask_hw, tuple(rendered.shape), tuple(gates.shape)
        loss, cosine_pos, cosine_neg = state.out[0].clone(), state.out[1].clone(), state.out[2].clone()
        ctx.mark_non_differentiable(cosine_pos, cosine_neg, state.selected)      # the logged cosines are taken under no_grad in the reference
        return loss, cosine_pos, cosine_neg, state.selected

    @staticmethod
    def backward(ctx, v_loss, _v_pos, _v_neg, _v_selected):
        F, selected, sel_counts, pixel_index, gates, labels, a = ctx.saved_tensors
        state = SeganyLossState(None, F, selected, sel_counts, None)
        _, v_gates, v_rendered = segany_loss_backward(state, ctx.rendered_shape, ctx.mask_hw, pixel_index, gates, labels, a,
                                                      v_loss.to(torch.float32).reshape(1).contiguous(), need_rendered=ctx.needs_input_grad[0])
        return v_rendered, v_gates.reshape(ctx.gates_shape) if ctx.needs_input_grad[1] else None, None, None, None, None, None, None


def segany_correspondence_loss(rendered: Tensor, mask_hw, pixel_index: Tensor, gates: Tensor, labels: Tensor, counts: Tensor, a: Tensor,
                               rand: Tensor, return_selected: bool = False):
    """rendered [C, Hr, Wr] (the renderer's map, channels first), mask_hw = (mh, mw), pixel_index [S] flat raster-order indices into the
    mask-sized grid, gates [Ns, C], labels / counts from segany_pair_labels, a [S] = mean_size at the sampled pixels, rand [S, S] (the
    draw the reference takes with rand_like) -> (loss, cosine_pos, cosine_neg), scalars on the device, and with `return_selected` the
    byte map [S, S] of the selection (bit 0 in M+, bit 1 in M-).

    The loss is the reference's without its norm regulariser: the features are the bilinear samples of `rendered` at the sampled mask
    pixels (F.interpolate, align_corners=False; the mask-sized map is never made), gated and normalised per scale; the pair weight is
    formed in the kernel.  The gradient reaches `rendered` and `gates`; the selection and the hard-sample flags carry none.  IEEE
    throughout: an empty selection gives NaN, as torch's mean of nothing does.  CPU tensors raise RuntimeError: there is no fallback."""
    who = "segany_correspondence_loss"
    _loss_inputs(who, rendered, mask_hw, pixel_index, gates, labels, counts, a, rand)
    mask_hw = (int(mask_hw[0]), int(mask_hw[1]))
    loss, cos_pos, cos_neg, selected = _SeganyLossFn.apply(rendered, gates, mask_hw, pixel_index.detach(), labels, counts, a.detach(), rand)
    return (loss, cos_pos, cos_neg, selected) if return_selected else (loss, cos_pos, cos_neg)

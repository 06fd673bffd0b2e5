"""The per-Gaussian appearance MLP of the appearance-embedding route, fused into one launch forward and one launch plus an ordered
reduce backward (internal/renderers/gsplat_appearance_embedding_renderer.py:50-93 with `tcnn: false`; include/gspl_hip.h section 21,
csrc/appearance.hip).

  appearance_mlp(features, weights, biases, embedding, *, mask=None, means=None, camera_center=None, n_view_frequencies=0,
                 normalize=False, output_activation="sigmoid") -> [N, n_out]
      act(W_last relu(... relu(W_0 [f^ | e^ | enc(d)] + b_0) ...) + b_last) for the rows the mask keeps, zeros for the others;
      differentiable in features, weights, biases and embedding.  No host synchronisation: the row count stays on the device.
  appearance_mlp_check(...): the host-side refusal of what is not built (NotImplementedError naming the option); CPU-callable.
  appearance_mlp_forward / appearance_mlp_backward: the launches alone, outside autograd.
  ROW_TILE, ROWS_PER_PASS, GRID_SIZE: rows of a wave tile, rows of a workgroup pass, workgroups at most (the kernel's constants).

GPU only, float32, exact fp32 arithmetic; no fallback here (the model module gspl_amd.appearance has the torch path for
configurations that are not built)."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch
from torch import Tensor

from .. import _lib as L
from . import _args as A
from ._common import _guarded

ROW_TILE = 32            # AP_TILE: rows of one wave tile (the MFMA's N)
ROWS_PER_PASS = 256      # AP_BLOCK: rows a workgroup compacts per pass
GRID_SIZE = 256          # AP_GRID: workgroups at most; the backward writes one partial per workgroup
LDS_BYTES = 160 * 1024
MAX_EMBEDDING_DIMS = 256
MAX_VIEW_FREQUENCIES = 8
NEURONS = (32, 64)
ACTIVATIONS = ("sigmoid", "none")
_NORMALIZE, _SIGMOID = 1, 2


def view_encoding_dims(n_view_frequencies: int) -> int:
    return 3 * (2 * int(n_view_frequencies) + 1) if int(n_view_frequencies) > 0 else 0


def lds_bytes(n_features: int, n_neurons: int, n_layers: int, n_view_frequencies: int, backward: bool, n_waves: int = 4) -> int:
    """The LDS a workgroup needs (ApGeom of csrc/appearance.hip): one image per layer with an odd stride, the biases, the embedding,
    the compaction list, and per wave the first layer's input tile and, in the backward, the two transpose tiles."""
    kb1 = -(-(int(n_features) + view_encoding_dims(n_view_frequencies)) // 32)
    hb = int(n_neurons) // 32
    floats = 0
    for layer in range(n_layers):
        rows = 32 * (1 if layer == n_layers - 1 else hb)
        floats += rows * (32 * (kb1 if layer == 0 else hb) + 1)
    floats += 64 * n_layers + MAX_EMBEDDING_DIMS + 2 * ROWS_PER_PASS + 8
    per_wave = 32 * (32 * kb1 + 1) + ((32 * (32 * hb + 1) + 32 * hb * 33) if backward else 0)
    return 4 * (floats + n_waves * per_wave)


def appearance_mlp_check(n_features: int, n_embedding_dims: int, n_neurons: int, n_layers: int, n_out: int, n_view_frequencies: int = 0,
                         output_activation: str = "sigmoid", skip_layers: Sequence[int] = (), dtype=torch.float32) -> None:
    """Raises NotImplementedError naming the first option the fused kernel is not built for; returns None when it is built."""
    if len(tuple(skip_layers)):
        raise NotImplementedError(f"appearance_mlp: skip_layers {list(skip_layers)} is not built (no skip connections in the fused kernel)")
    if dtype != torch.float32:
        raise NotImplementedError(f"appearance_mlp: dtype {dtype} is not built; float32 only")
    if n_features % 4 or not 4 <= n_features <= 128:
        raise NotImplementedError(f"appearance_mlp: n_gaussian_feature_dims must be a multiple of 4 in 4 .. 128, got {n_features}")
    if not 0 <= n_embedding_dims <= MAX_EMBEDDING_DIMS:
        raise NotImplementedError(f"appearance_mlp: n_appearance_embedding_dims must be at most {MAX_EMBEDDING_DIMS}, got {n_embedding_dims}")
    if n_neurons not in NEURONS:
        raise NotImplementedError(f"appearance_mlp: n_neurons must be one of {NEURONS}, got {n_neurons}")
    if not 2 <= n_layers <= 4:
        raise NotImplementedError(f"appearance_mlp: n_layers must be 2 .. 4, got {n_layers}")
    if n_out not in (3, 4):
        raise NotImplementedError(f"appearance_mlp: n_out must be 3 or 4, got {n_out}")
    if not 0 <= n_view_frequencies <= MAX_VIEW_FREQUENCIES:
        raise NotImplementedError(f"appearance_mlp: n_view_direction_frequencies must be 0 .. {MAX_VIEW_FREQUENCIES}, got {n_view_frequencies}")
    if output_activation not in ACTIVATIONS:
        raise NotImplementedError(f"appearance_mlp: output_activation must be one of {ACTIVATIONS}, got {output_activation!r}")
    if lds_bytes(n_features, n_neurons, n_layers, n_view_frequencies, True, 1) > LDS_BYTES:
        raise NotImplementedError(f"appearance_mlp: the weights of n_gaussian_feature_dims {n_features} with n_view_direction_frequencies "
                                  f"{n_view_frequencies} exceed the LDS budget of {LDS_BYTES} bytes")


class _Net:
    """The arguments both launches share, checked: shapes of a call and the host arrays of layer pointers (kept alive here)."""

    def __init__(self, features: Tensor, weights, biases, embedding: Tensor, mask, means, camera_center, n_view_frequencies, normalize,
                 output_activation):
        self.N, self.F = features.shape
        self.E = embedding.numel()
        self.n_layers = len(weights)
        self.H = weights[0].shape[0]
        self.n_out = weights[-1].shape[0]
        self.n_freq = int(n_view_frequencies)
        self.flags = (_NORMALIZE if normalize else 0) | (_SIGMOID if output_activation == "sigmoid" else 0)
        self.features, self.embedding, self.weights, self.biases = features, embedding, list(weights), list(biases)
        self.mask, self.means, self.camera_center = mask, means, camera_center
        self._w = (ctypes.c_void_p * self.n_layers)(*[w.data_ptr() for w in self.weights])
        self._b = (ctypes.c_void_p * self.n_layers)(*[b.data_ptr() for b in self.biases])
        self.n_params = sum(w.numel() + b.numel() for w, b in zip(self.weights, self.biases)) + self.E

    def head(self):
        return (self.N, self.F, self.E, self.H, self.n_layers, self.n_out, self.n_freq, self.flags, L.ptr(self.features, torch.float32),
                L.ptr(self.mask, torch.uint8), L.ptr(self.means, torch.float32), L.ptr(self.camera_center, torch.float32),
                L.ptr(self.embedding, torch.float32), ctypes.cast(self._w, ctypes.c_void_p), ctypes.cast(self._b, ctypes.c_void_p))


@_guarded(0)
def appearance_mlp_forward(features: Tensor, weights, biases, embedding: Tensor, mask: Optional[Tensor] = None, means: Optional[Tensor] = None,
                           camera_center: Optional[Tensor] = None, n_view_frequencies: int = 0, normalize: bool = False,
                           output_activation: str = "sigmoid", out: Optional[Tensor] = None) -> Tensor:
    """The forward launch alone: contiguous float32 tensors on the GPU, mask uint8 -> out [N, n_out], every row written."""
    net = _Net(features, weights, biases, embedding, mask, means, camera_center, n_view_frequencies, normalize, output_activation)
    out = A.out("appearance_mlp_forward", "out", out, (net.N, net.n_out), torch.float32, features, contiguous=False)
    L.call("gspl_appearance_mlp_fwd", *net.head(), L.ptr(out), L.stream())
    return out


@_guarded(0)
def appearance_mlp_backward(features: Tensor, weights, biases, embedding: Tensor, v_out: Tensor, mask: Optional[Tensor] = None,
                            means: Optional[Tensor] = None, camera_center: Optional[Tensor] = None, n_view_frequencies: int = 0,
                            normalize: bool = False, output_activation: str = "sigmoid", want_features: bool = True, want_params: bool = True,
                            v_features: Optional[Tensor] = None, v_params: Optional[Tensor] = None):
    """The backward alone: v_out [N, n_out] -> (v_features [N, F] or None, v_params flat or None).  v_params holds
    [W_0 | b_0 | W_1 | b_1 | ... | embedding]; every element of both is written (masked rows of v_features as zeros).  `v_features`
    and `v_params` may be the caller's buffers.  want_params=False: no weight-gradient arithmetic and no reduce."""
    net = _Net(features, weights, biases, embedding, mask, means, camera_center, n_view_frequencies, normalize, output_activation)
    A.shape("appearance_mlp_backward", "v_out", v_out, (net.N, net.n_out))
    v = v_out.to(torch.float32).contiguous()
    dev = features.device
    if want_features and v_features is None:
        v_features = torch.empty((net.N, net.F), dtype=torch.float32, device=dev)
    if want_params and v_params is None:
        v_params = torch.empty((net.n_params,), dtype=torch.float32, device=dev)
    if not want_features:
        v_features = None
    workspace, ws_bytes = None, 0
    if want_params:
        if v_params.numel() != net.n_params or v_params.dtype != torch.float32:
            raise ValueError(f"appearance_mlp_backward: v_params must hold {net.n_params} float32")
        ws_bytes = L.lib().gspl_appearance_mlp_workspace_bytes(net.N, net.F, net.E, net.H, net.n_layers, net.n_out, net.n_freq)
        workspace = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    else:
        v_params = None
    if v_features is not None or v_params is not None:
        L.call("gspl_appearance_mlp_bwd", *net.head(), L.ptr(v), L.ptr(v_features), L.ptr(v_params), L.ptr(workspace), ws_bytes, L.stream())
    return v_features, v_params


def split_params(v_params: Tensor, weights, biases, n_embedding_dims: int):
    """Views of the flat gradient in the parameters' shapes: ([v_W_l], [v_b_l], v_embedding)."""
    v_w, v_b, at = [], [], 0
    for w, b in zip(weights, biases):
        v_w.append(v_params[at:at + w.numel()].view(w.shape))
        at += w.numel()
        v_b.append(v_params[at:at + b.numel()].view(b.shape))
        at += b.numel()
    return v_w, v_b, v_params[at:at + n_embedding_dims]


class _AppearanceMlpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, embedding, mask, means, camera_center, options, *params):
        n_layers = len(params) // 2
        fc, ec = features.detach().contiguous(), embedding.detach().contiguous()
        ws = [p.detach().contiguous() for p in params[:n_layers]]
        bs = [p.detach().contiguous() for p in params[n_layers:]]
        ctx.save_for_backward(fc, ec, *ws, *bs)
        ctx.side = (mask, means, camera_center)
        ctx.options, ctx.n_layers, ctx.embedding_shape = options, n_layers, embedding.shape
        return appearance_mlp_forward(fc, ws, bs, ec, mask, means, camera_center, *options)

    @staticmethod
    def backward(ctx, v_out):
        fc, ec, *params = ctx.saved_tensors
        n = ctx.n_layers
        ws, bs = params[:n], params[n:]
        want_features = ctx.needs_input_grad[0]
        want_params = ctx.needs_input_grad[1] or any(ctx.needs_input_grad[6:])
        mask, means, camera_center = ctx.side
        v_features, v_params = appearance_mlp_backward(fc, ws, bs, ec, v_out, mask, means, camera_center, *ctx.options,
                                                       want_features=want_features, want_params=want_params)
        grads = [None] * (2 * n)
        v_embedding = None
        if v_params is not None:
            v_w, v_b, v_e = split_params(v_params, ws, bs, ec.numel())
            grads = [g if need else None for g, need in zip(v_w + v_b, ctx.needs_input_grad[6:])]
            v_embedding = v_e.view(ctx.embedding_shape) if ctx.needs_input_grad[1] else None
        return (v_features, v_embedding, None, None, None, None, *grads)


def appearance_mlp(features: Tensor, weights: Sequence[Tensor], biases: Sequence[Tensor], embedding: Tensor, *, mask: Optional[Tensor] = None,
                   means: Optional[Tensor] = None, camera_center: Optional[Tensor] = None, n_view_frequencies: int = 0, normalize: bool = False,
                   output_activation: str = "sigmoid") -> Tensor:
    """features [N, F] float32 on the GPU; weights[l] [out, in] and biases[l] [out] as torch.nn.Linear keeps them, the first layer's
    `in` being F + E (+ 3 (2 n_view_frequencies + 1)) in the order features | embedding | encoded direction; embedding [E]: the one
    row this call uses; mask [N] bool or None -> [N, n_out] float32, rows the mask drops written as zeros.

    n_view_frequencies > 0: the kernel forms the direction (means[n] - camera_center) / max(|.|, 1e-12) itself (means [N, 3],
    camera_center [3], both on the device) and encodes it as x, sin(2^0 x), cos(2^0 x), sin(2^1 x), ...; it carries no gradient.
    normalize=True applies F.normalize (eps 1e-12) to each feature row and to the embedding, backward included.

    Gradients reach features (masked rows: zeros, written), every weight and bias, and the embedding; the parameter gradients are
    summed in a fixed order (no float atomics): two backward calls give the same bits.  Parameters that need no gradient cost no
    weight-gradient arithmetic.  Non-contiguous inputs are copied.  What is not built raises NotImplementedError naming the option
    before any launch; CPU tensors raise RuntimeError: there is no fallback here."""
    who, weights, biases = "appearance_mlp", list(weights), list(biases)
    named = ([("features", features), ("embedding", embedding)] + [(f"weights[{i}]", w) for i, w in enumerate(weights)]
             + [(f"biases[{i}]", b) for i, b in enumerate(biases)])
    for name, t in named:
        A.tensor(who, name, t)
    if features.dim() != 2:
        raise ValueError(f"appearance_mlp: features must be [N, F], got {tuple(features.shape)}")
    if len(weights) != len(biases) or not weights:
        raise ValueError(f"appearance_mlp: {len(weights)} weights for {len(biases)} biases")
    if any(w.dim() != 2 for w in weights) or any(b.dim() != 1 for b in biases):
        raise ValueError("appearance_mlp: weights must be [out, in] and biases [out]")
    N, F = features.shape
    E, H, n_out, n_layers = embedding.numel(), weights[0].shape[0], weights[-1].shape[0], len(weights)
    dtypes = {t.dtype for t in [features, embedding] + weights + biases}
    appearance_mlp_check(F, E, H, n_layers, n_out, int(n_view_frequencies), output_activation,
                         dtype=next(iter(dtypes - {torch.float32}), torch.float32))
    P = view_encoding_dims(n_view_frequencies)
    for layer, (w, b) in enumerate(zip(weights, biases)):
        want = (n_out if layer == n_layers - 1 else H, F + E + P if layer == 0 else H)
        if tuple(w.shape) != want:
            if layer and w.shape[1] != H:
                raise NotImplementedError(f"appearance_mlp: layer {layer} reads {w.shape[1]} inputs; skip_layers and other widths are not built")
            raise ValueError(f"appearance_mlp: weights[{layer}] must be {list(want)}, got {list(w.shape)}")
        if b.shape[0] != want[0]:
            raise ValueError(f"appearance_mlp: biases[{layer}] must be [{want[0]}], got {list(b.shape)}")
    for name, t in named:
        A.on_gpu(who, name, t, features, "features")
    if N >= 2 ** 31 - ROWS_PER_PASS:
        raise ValueError(f"appearance_mlp: features has {N} rows; fewer than 2^31 - {ROWS_PER_PASS} are built")
    if mask is not None:
        if mask.dtype != torch.bool or tuple(mask.shape) != (N,) or mask.device != features.device:
            raise ValueError(f"appearance_mlp: mask must be bool [{N}] on {features.device}, got {mask.dtype} {tuple(mask.shape)}")
        mask = mask.contiguous().view(torch.uint8)
    if P:
        if means is None or camera_center is None:
            raise ValueError("appearance_mlp: n_view_frequencies > 0 needs means and camera_center")
        if tuple(means.shape) != (N, 3) or camera_center.numel() != 3:
            raise ValueError(f"appearance_mlp: means must be [{N}, 3] and camera_center [3]")
        A.on_gpu(who, "means", means)
        A.on_gpu(who, "camera_center", camera_center)      # (it stays on the device)
        means = means.detach().to(torch.float32).contiguous()
        camera_center = camera_center.detach().to(torch.float32).reshape(3).contiguous()
    else:
        means = camera_center = None
    options = (int(n_view_frequencies), bool(normalize), output_activation)
    return _AppearanceMlpFn.apply(features, embedding.reshape(-1), mask, means, camera_center, options, *weights, *biases)

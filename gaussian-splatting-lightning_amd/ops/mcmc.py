"""The 3DGS-MCMC density controller's math (Kheradmand et al., "3D Gaussian Splatting as Markov Chain Monte Carlo"): one C-ABI
call each (include/gspl_hip.h section 13, csrc/mcmc.hip).

  compute_relocation(opacities, scales, ratios, binoms)   `gsplat.relocation.compute_relocation` (reference call site
      internal/density_controllers/mcmc_density_controller.py:121-128): same signature, same returns.  One difference: gsplat
      clamps `ratios` to [1, n_max] IN PLACE; here the caller's tensor is left as it is (the kernel clamps in registers).
  perturb_means_(means, scales, rotations, opacities, ...)  the whole of `MCMCDensityControllerImpl._add_xyz_noise` (:93-119) in
      one launch, with its normal draws made inside the kernel (Philox4x32-10 keyed by the device's torch generator).
  mcmc_regularization(opacities, scales, opacity_w, scale_w, raw=...)   `MCMCMetricsModuleMixin.reg_loss`'s two weighted means
      (internal/metrics/mcmc_metrics.py), forward and backward.

GPU only, float32, contiguous; no fallback."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _lib as L
from . import _args as A
from ._common import _guarded, join_pending_updates
from ._state import STATE as S


def _flat_rows(*rows):
    """(name, tensor or None, elements) each: float32 on the GPU, contiguous, of that many elements whatever the shape."""
    for name, t, n in rows:
        if t is not None:
            A.numel(None, name, A.contiguous(None, name, A.gpu_f32("MCMC", name, t)), n)


@torch.no_grad()
def compute_relocation(opacities: Tensor, scales: Tensor, ratios: Tensor, binoms: Tensor) -> Tuple[Tensor, Tensor]:
    """new_opacities [M], new_scales [M,3] of Eq. 9 for each row with n = clamp(ratios, 1, n_max) copies (header section 13).
    opacities [M] and scales [M,3] are activated values; ratios of any integer dtype; binoms [n_max, n_max] (binoms[n,k] = C(n,k))."""
    M = opacities.shape[0] if opacities.dim() > 0 else 1
    _flat_rows(("opacities", opacities, M), ("scales", scales, 3 * M))
    if not binoms.dim() == 2 or binoms.shape[0] != binoms.shape[1]:
        raise ValueError(f"binoms must be [n_max, n_max], got {tuple(binoms.shape)}")
    n_max = int(binoms.shape[0])
    _flat_rows(("binoms", binoms, n_max * n_max))
    A.on_gpu(None, "ratios", ratios, family="MCMC")
    if ratios.dtype.is_floating_point or ratios.dtype == torch.bool or ratios.numel() != M:
        raise ValueError(f"ratios: {M} integers expected, got {ratios.numel()} of {ratios.dtype}")
    A.contiguous(None, "ratios", ratios)
    if ratios.dtype != torch.int32:
        ratios = ratios.clamp(1, n_max).to(torch.int32)       # a new tensor: the caller's stays as it is
    new_opacities = torch.empty((M,), dtype=torch.float32, device=opacities.device)
    new_scales = torch.empty((M, 3), dtype=torch.float32, device=opacities.device)
    if M == 0:
        return new_opacities, new_scales
    with L.device_guard(opacities):
        L.call("gspl_mcmc_relocation", M, n_max, L.ptr(opacities), L.ptr(scales), L.ptr(ratios), L.ptr(binoms), L.ptr(new_opacities),
               L.ptr(new_scales), L.stream())
    return new_opacities, new_scales


OFFSET_STEP = 4      # generator offset consumed per noise call (one Philox block per Gaussian; a multiple of 4 as torch's own kernels use)


def _generator(device, generator: Optional[torch.Generator]) -> torch.Generator:
    if generator is not None:
        return generator
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return torch.cuda.default_generators[idx]


def next_noise_key(device, generator: Optional[torch.Generator] = None) -> Tuple[int, int]:
    """(seed, offset) of the next noise call on `device`, and advance the generator's offset past it.  The kernel draws the first Philox
    block of curand_init(seed, subsequence = row, offset), the block torch's own kernels would draw for offsets [offset, offset + 4);
    reserving those offsets means that no other draw of this generator — a noise call or a torch kernel — uses the same block.
    `torch.manual_seed` reproduces a run, and nothing is read from the device (the state lives on the host)."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("perturb_means_: refusing to draw noise while a CUDA graph is being captured (the key would be baked in)")
    g = _generator(device, generator)
    seed, offset = int(g.initial_seed()), int(g.get_offset())
    offset = (offset + 3) // 4 * 4            # torch advances by multiples of 4; round up in case something did not
    g.set_offset(offset + OFFSET_STEP)
    return seed & 0xFFFFFFFFFFFFFFFF, offset


@torch.no_grad()
def perturb_means_(means: Tensor, scales: Tensor, rotations: Tensor, opacities: Tensor, *, raw: bool, noise_scale: float,
                   noise: Optional[Tensor] = None, generator: Optional[torch.Generator] = None) -> Tensor:
    """means += noise_scale / (1 + exp(-100 ((1 - o) - 0.995))) R(q) diag(s^2) R(q)^T eps, in place; returns `means`.
    raw=True: scales / rotations / opacities are the model's raw parameters (exp / normalize / sigmoid applied inside, see
    renderers.renderer.model_raw_parameters); raw=False: the activated getters' values.  noise_scale = noise_lr * the means' lr.
    eps [N,3] given in `noise`, or drawn inside the kernel from `generator` (default: the device's torch generator)."""
    N = means.shape[0]
    _flat_rows(("means", means, 3 * N), ("scales", scales, 3 * N), ("rotations", rotations, 4 * N), ("opacities", opacities, N),
               ("noise", noise, 3 * N))
    if N == 0:
        return means
    if S.pending_updates:
        join_pending_updates(means.device)      # a parameter update may still be in flight on the colour stream
    seed, offset = (0, 0) if noise is not None else next_noise_key(means.device, generator)
    with L.device_guard(means):
        L.call("gspl_mcmc_perturb_means", N, int(bool(raw)), L.ptr(means), L.ptr(scales), L.ptr(rotations), L.ptr(opacities), L.ptr(noise),
               float(noise_scale), seed, offset, L.stream())
    return means


@torch.no_grad()
def mcmc_randn(n: int, seed: int, offset: int, device, bits: bool = False):
    """The noise generator of perturb_means_ on its own (tests): normals [n,3] (and the Philox words u32 [n,4] as int32)."""
    normals = torch.empty((n, 3), dtype=torch.float32, device=device)
    words = torch.empty((n, 4), dtype=torch.int32, device=device) if bits else None
    if n > 0:
        with L.device_guard(normals):
            L.call("gspl_mcmc_randn", n, int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF, L.ptr(words), L.ptr(normals), L.stream())
    return (normals, words) if bits else normals


class _MCMCRegFn(torch.autograd.Function):
    @staticmethod
    @_guarded(1)
    def forward(ctx, opacities, scales, opacity_w, scale_w, raw):
        N = opacities.numel()
        _flat_rows(("opacities", opacities, N), ("scales", scales, 3 * N))
        out = torch.zeros((2,), dtype=torch.float32, device=opacities.device)
        if N > 0:
            partials = torch.empty((2 * L.lib().gspl_mcmc_reg_partials(N),), dtype=torch.float32, device=opacities.device)
            L.call("gspl_mcmc_reg_fwd", N, int(bool(raw)), L.ptr(opacities), L.ptr(scales), float(opacity_w), float(scale_w), L.ptr(partials),
                   L.ptr(out), L.stream())
        ctx.save_for_backward(opacities, scales)
        ctx.cfg = (float(opacity_w), float(scale_w), int(bool(raw)))
        return out

    @staticmethod
    @_guarded(0)
    def backward(ctx, grad_out):
        opacities, scales = ctx.saved_tensors
        opacity_w, scale_w, raw = ctx.cfg
        v_o, v_s = torch.empty_like(opacities), torch.empty_like(scales)
        N = opacities.numel()
        if N > 0:
            g = grad_out.float().contiguous()
            L.call("gspl_mcmc_reg_bwd", N, raw, L.ptr(opacities), L.ptr(scales), opacity_w, scale_w, L.ptr(g), L.ptr(v_o), L.ptr(v_s),
                   L.stream())
        return v_o, v_s, None, None, None


def mcmc_regularization(opacities: Tensor, scales: Tensor, opacity_w: float, scale_w: float, *, raw: bool) -> Tuple[Tensor, Tensor]:
    """(opacity_w * mean|f(opacities)|, scale_w * mean|g(scales)|) as two 0-d tensors that carry gradients to both inputs;
    f, g = sigmoid, exp on raw parameters, the identity on activated ones.  N = 0 gives two zeros."""
    out = _MCMCRegFn.apply(opacities, scales, opacity_w, scale_w, raw)
    return out[0], out[1]

"""The argument checks of the route ops: one function per check.  Each takes `who` (the op's name as its messages state it) and
`name` (the argument), and raises, or returns the tensor.  A module's check is a short sequence of these calls in that module's own
order; no module formats these sentences itself.

The order that lets a machine without a GPU meet every refusal: types (TypeError), shapes (ValueError), dtypes, and the device last
(RuntimeError), because a CPU tensor stops at the device check.  glossy and lod follow it; the older modules ask for the device
first, and keep doing so: the order decides what a caller sees.

The older families (mesh, surface, bilagrid, MCMC, PVG, environment light) name no op in their messages: they pass who=None and the
sentences start with the argument, as their tests pin them ("tsdf: the mesh ops run on the GPU only", "depth: float32 is needed")."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch
from torch import Tensor


def _head(who: Optional[str], name: str) -> str:
    return f"{who}: {name}" if who else name


def _dt(dtype) -> str:
    return str(dtype).replace("torch.", "")


def tensor(who, name, t) -> Tensor:
    if not isinstance(t, Tensor):
        raise TypeError(f"{_head(who, name)} must be a tensor, got {type(t).__name__}")
    return t


def on_gpu(who, name, t, like: Optional[Tensor] = None, like_name: Optional[str] = None, family: Optional[str] = None) -> Tensor:
    """A CPU tensor (or, where `tensor` was not asked first, anything that is no tensor) is refused; so is a device other than
    `like`'s.  `family`: the older modules' wording, "the mesh ops run on the GPU only"."""
    if not isinstance(t, Tensor) or not t.is_cuda:
        where = f": the {family} ops run on the GPU only" if family else " must be on the GPU"
        raise RuntimeError(f"{_head(who, name)}{where}; there is no CPU fallback")
    if like is not None and t.device != like.device:
        raise RuntimeError(f"{_head(who, name)} is on {t.device}, {like_name or 'not'} on {like.device}")
    return t


def dtype(who, name, t: Tensor, *dtypes, error=NotImplementedError) -> Tensor:
    """`error` exists because the classes differ and callers may rely on them: RuntimeError in mesh, surface, bilagrid, mcmc, knn and
    hashgrid; NotImplementedError in hexplane, glossy, lod, spotless and segany."""
    if t.dtype not in dtypes:
        want = " or ".join(_dt(d) for d in dtypes)
        raise error(f"{who}: {name} must be {want}, got {t.dtype}" if who else f"{name}: {want} is needed, got {t.dtype}")
    return t


def gpu_tensor(who, name, t, *dtypes, like: Optional[Tensor] = None, like_name: Optional[str] = None) -> Tensor:
    """segany's and spotless' one check, in their order: a tensor, on the GPU, on `like`'s device, of one of `dtypes`."""
    return dtype(who, name, on_gpu(who, name, tensor(who, name, t), like, like_name), *dtypes)


def gpu_f32(family, name, t, want=None, like: Optional[Tensor] = None, like_name: Optional[str] = None) -> Tensor:
    """The older families' one check, in their order: on the GPU, float32 (a RuntimeError there), the shape, `like`'s device."""
    dtype(None, name, on_gpu(None, name, t, family=family), torch.float32, error=RuntimeError)
    if want is not None:
        shape(None, name, t, want)
    return t if like is None else on_gpu(None, name, t, like, like_name)


def shape(who, name, t: Tensor, shape) -> Tensor:
    """An entry of `shape` that is no integer (None, or a letter for the message) matches any extent."""
    if t.dim() != len(shape) or any(isinstance(w, int) and w != g for w, g in zip(shape, t.shape)):
        want = ", ".join("N" if w is None else str(w) for w in shape)
        raise ValueError(f"{_head(who, name)} must be [{want}], got {list(t.shape)}")
    return t


def numel(who, name, t: Tensor, n: int) -> Tensor:
    if t.numel() != n:
        raise ValueError(f"{_head(who, name)} must hold {n} element(s), got {t.numel()} (shape {list(t.shape)})")
    return t


def contiguous(who, name, t: Tensor, error=RuntimeError) -> Tensor:
    if not t.is_contiguous():
        raise error(f"{_head(who, name)} must be contiguous")
    return t


def aligned16(who, name, t: Tensor) -> Tensor:
    """Of contiguous tensors only: a non-contiguous one is copied before it is read, and the copy is aligned."""
    if t.is_contiguous() and t.data_ptr() % 16:
        raise ValueError(f"{_head(who, name)} must be aligned to 16 bytes (a view into the middle of another tensor?)")
    return t


def out(who, name, t: Optional[Tensor], shape, dtype, like: Tensor, contiguous: bool = True) -> Tensor:
    """The caller's buffer (checked as `buffer` does), or a new one when there is none."""
    return torch.empty(shape, dtype=dtype, device=like.device) if t is None else buffer(who, name, t, shape, dtype, like, contiguous)


def buffer(who, name, t, shape, dtype, like: Tensor, contiguous: bool = True) -> Tensor:
    """A buffer of the caller's: of `shape` (a tuple, or an integer where only the element count is fixed) and `dtype`, on `like`'s
    device.  contiguous=False where the module never asked (`_lib.ptr` refuses such a buffer later, in its own words)."""
    fits = isinstance(t, Tensor) and (t.numel() == shape if isinstance(shape, int) else tuple(t.shape) == tuple(shape))
    if not fits or t.dtype != dtype or t.device != like.device or (contiguous and not t.is_contiguous()):
        want = f"{shape} values" if isinstance(shape, int) else list(shape)
        got = f"{_dt(t.dtype)} {list(t.shape)} on {t.device}" if isinstance(t, Tensor) else type(t).__name__
        raise ValueError(f"{_head(who, name)} must be {'contiguous ' if contiguous else ''}{_dt(dtype)} {want} on {like.device}, got {got}")
    return t


def rows16(v: Tensor) -> Tensor:
    """An incoming gradient as the row kernels read it: float32, contiguous, 16-byte aligned (a clone when it is not)."""
    v = v.to(torch.float32).contiguous()
    return v.clone() if v.data_ptr() % 16 else v


def host_ptr(a):
    """The address of a numpy array the library reads on the host."""
    return ctypes.c_void_p(a.ctypes.data)


def raw_ptr(t: Optional[Tensor]):
    """Device pointer of a possibly non-contiguous tensor's first element."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())

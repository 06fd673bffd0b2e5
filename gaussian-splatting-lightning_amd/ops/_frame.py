"""The library's allocation call-back (`gspl_alloc_fn`, include/gspl_hip.h section 6b): the one place where torch-owned memory and the raw
device addresses the library keeps in `gspl_inria_state` / `gspl_surfel_state` meet.

A call that allocates through the library runs inside `with FrameBlocks(device) as frame:` and is handed `frame.callback`.  The blocks
the state points into are saved tensors of the autograd node (`frame.saved()`): autograd frees them with the graph.  The backward gets
them back through `frame.unpack(...)`, which refuses blocks that no longer live where the state points before anything is launched."""
from __future__ import annotations

import math
import threading

import torch
from torch import Tensor

from .. import _lib as L

# blocks no kernel reads after the call that asked for them
_SCRATCH = (L.GSPL_BUF_BINNING, L.GSPL_BUF_LISTS_WORK, L.GSPL_BUF_SURFEL_ENTRIES)
_CURRENT = threading.local()      # .frame: the FrameBlocks of the library call running on this thread


def allocate(nbytes: int, device, tag: int) -> Tensor:
    """One block of device memory for the library; `tag` (GSPL_BUF_*) says what it is for.  The trampoline looks this function up per
    block: tests replace it."""
    return torch.empty((nbytes,), dtype=torch.uint8, device=device)


def _trampoline(_ctx, tag, nbytes):
    frame = _CURRENT.frame
    try:
        t = allocate(max(int(nbytes), 1), frame.device, tag)
    except Exception as e:      # an exception must not cross the C boundary: NULL = failure, re-raised by FrameBlocks
        frame.error = e
        return 0
    frame.asked.setdefault(tag, []).append(t)
    return t.data_ptr()


_CALLBACK = L.ALLOC_FN(_trampoline)      # (referenced for the life of the process: ctypes frees a call-back with its object)


class Blocks:
    """Byte blocks the library carved up."""

    def __init__(self, tensors):
        self.tensors = list(tensors)

    def view(self, address: int, shape, dtype) -> Tensor:
        """Typed view of the region at device address `address` in the block that holds it (`.data`: writes through the view do not
        move a saved tensor's version counter)."""
        nbytes = math.prod(shape) * dtype.itemsize
        for t in self.tensors:
            off = address - t.data_ptr()
            if 0 <= off and off + nbytes <= t.numel():
                return t.data[off:off + nbytes].view(dtype).view(shape)
        raise RuntimeError(f"no block of the frame holds {nbytes} bytes at {address:#x}")


class FrameBlocks(Blocks):
    """The blocks of one library call.  After the call the scratch blocks are dropped and of every other tag the last block is kept: a
    block asked for a second time (the speculative list length was too low) replaces the first."""

    callback = _CALLBACK

    def __init__(self, device):
        super().__init__(())
        self.device = device
        self.asked = {}            # tag -> [blocks], while the call runs
        self.error = None          # what `allocate` raised
        self.kept = {}             # tag -> the block kept, until `saved()`
        self.addresses = {}        # tag -> its device address

    def __enter__(self):
        _CURRENT.frame = self
        return self

    def __exit__(self, exc_type, exc, tb):
        _CURRENT.frame = None
        asked, error = self.asked, self.error
        self.asked, self.error = {}, None
        if exc_type is not None:
            if issubclass(exc_type, RuntimeError) and error is not None:
                raise error      # the library's "allocation call-back returned NULL" was this
            return False
        # (after a call that succeeded a refused block is no error: the library does without checkpoints it could not get)
        self.kept = {tag: ts[-1] for tag, ts in asked.items() if tag not in _SCRATCH}
        self.tensors = list(self.kept.values())
        self.addresses = {tag: t.data_ptr() for tag, t in self.kept.items()}
        return False

    def saved(self) -> list:
        """The kept blocks, for `ctx.save_for_backward`.  From here on autograd owns them and this object keeps their addresses only."""
        tensors, self.tensors, self.kept = self.tensors, [], {}
        return tensors

    def unpack(self, saved) -> Blocks:
        """The backward's blocks (`saved`: what `saved()` returned, as the node unpacked it).  They must live where the forward's state
        points: saved-tensor hooks (torch.autograd.graph.save_on_cpu, non-reentrant torch.utils.checkpoint) hand the backward copies at
        other addresses while the originals went back to the allocator."""
        if [t.data_ptr() for t in saved] != list(self.addresses.values()):
            raise RuntimeError("the frame's device blocks moved between forward and backward (saved-tensor hooks such as "
                               "torch.autograd.graph.save_on_cpu or non-reentrant checkpointing): the rasterizer's state points into "
                               "the forward's blocks, so its backward cannot run under such hooks")
        return Blocks(saved)

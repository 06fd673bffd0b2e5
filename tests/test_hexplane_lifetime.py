"""Buffer lifetime of the HexPlane op, in the style of tests/test_guard_bands.py: out, v_table and v_x sit between poisoned bands inside
one plain tensor; forward and backward leave the bands as they were, and what they write does not depend on what the buffers held
before (0xFF bytes, NaN patterns, or zeros)."""
import numpy as np
import pytest
import torch

from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 1024          # floats


def _run(F, L, N, fill_byte, per_point_time):
    from gspl_amd import ops
    lay = ops.hexplane_layout([5, 6, 7, 3], [1, 2, 4, 8][:L], F)
    n_out, n_table, n_x = N * lay.n_output_dims, lay.n_params, N * 3
    pad = lambda n: (-n) % 4                                   # keeps the next slot on a 16-byte boundary
    sizes = [n_out, n_table, n_x]
    starts, at = [], BAND
    for n in sizes:
        starts.append(at)
        at += n + pad(n) + BAND
    arena = torch.empty((at,), dtype=torch.float32, device=DEV)
    poison = torch.tensor(0x7FC0DEAD, dtype=torch.int32, device=DEV)
    arena.view(torch.int32).fill_(poison)
    out = arena[starts[0]:starts[0] + n_out].view(N, lay.n_output_dims)
    v_table = arena[starts[1]:starts[1] + n_table]
    v_x = arena[starts[2]:starts[2] + n_x].view(N, 3)
    out.view(torch.uint8).fill_(fill_byte)
    v_x.view(torch.uint8).fill_(fill_byte)
    v_table.zero_()                                            # accumulated into: the caller clears it
    rng = np.random.default_rng(31)
    x = torch.from_numpy(((rng.random((N, 3), dtype=np.float32) * 2 - 1) * 3).astype(np.float32)).to(DEV)          # inside and outside the box
    t = torch.from_numpy(((rng.random(N, dtype=np.float32) * 2 - 1) * 1.5).astype(np.float32)).to(DEV) if per_point_time else 0.625
    table = torch.from_numpy((rng.random((lay.total, F), dtype=np.float32) + 0.1).astype(np.float32)).to(DEV)
    v_out = torch.from_numpy(rng.standard_normal((N, lay.n_output_dims)).astype(np.float32)).to(DEV)
    box = ops.hexplane_box(np.array([[2.0] * 3, [-2.0] * 3], dtype=np.float32))
    ops.hexplane_forward(x, t, table, box, lay, out=out)
    ops.hexplane_backward(x, t, table, box, lay, v_out, v_table, v_x=v_x)
    torch.cuda.synchronize()
    words = arena.view(torch.int32)
    edges = [0] + [e for s, n in zip(starts, sizes) for e in (s, s + n)] + [arena.numel()]
    for lo, hi in zip(edges[0::2], edges[1::2]):
        assert bool((words[lo:hi] == poison).all()), f"the band [{lo}, {hi}) was written"
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(v_table).all()) and bool(torch.isfinite(v_x).all())
    assert bool(v_table.any()) and bool(v_x.any())
    return out.clone(), v_x.clone()


@pytest.mark.parametrize("F,L,N,per_point_time", [(8, 1, 333, True), (32, 2, 333, False), (64, 4, 61, True)])
def test_guard_bands_stay_intact_and_prefill_does_not_matter(F, L, N, per_point_time):
    out_ff, v_x_ff = _run(F, L, N, 0xFF, per_point_time)
    out_00, v_x_00 = _run(F, L, N, 0x00, per_point_time)
    assert torch.equal(out_ff, out_00) and torch.equal(v_x_ff, v_x_00)

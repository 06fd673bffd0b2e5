"""Exit discipline of the fused forward calls (csrc/fused.hip, csrc/surfel.hip) at the C boundary: whichever allocation call-back the
caller refuses, in each of the three list-building regimes, the call either ends with that refusal or does without the block, the
stream stays healthy, and the next frame is bit-equal to the first.  Every refusal is an error code from the host: no path here
faults the device."""
import ctypes

import pytest
import torch

from oracle import gsplat_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, W, H = 500, 70, 50      # a 5 x 4 tile grid whose last column and row are partial


def _inputs():
    means, scales, quats, opac, shs = O.synthetic_scene(N, seed=31)
    cam = O.synthetic_camera(W, H, 64.0)
    t = lambda x: x.to(DEV).contiguous()
    return {"means": t(means), "scales": t(scales * 4), "quats": t(quats), "opac": t(opac.reshape(-1)), "shs": t(shs),
            "view": t(cam["world_to_camera"]), "proj": t(cam["full_projection"]), "campos": t(cam["camera_center"]),
            "bg": t(torch.tensor([0.1, 0.3, 0.6])), "tanx": float(cam["tanfovx"]), "tany": float(cam["tanfovy"])}


def _inria(x, hint):
    from gspl_amd import _lib as L
    from gspl_amd.ops import _frame
    state = L.InriaState()
    state.flags = L.GSPL_INRIA_WILL_BACKWARD | L.GSPL_INRIA_FORCE_SEGMENTS
    out, radii = torch.empty(3, H, W, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV)
    with _frame.FrameBlocks(DEV) as frame:
        L.call("gspl_rasterize_inria_fwd", N, 3, 16, L.ptr(x["means"]), L.ptr(x["scales"]), L.ptr(x["quats"]), None, L.ptr(x["shs"]), None, None,
               L.ptr(x["opac"]), L.ptr(x["view"]), L.ptr(x["proj"]), L.ptr(x["campos"]), L.ptr(x["bg"]), W, H, x["tanx"], x["tany"], 1.0,
               frame.callback, None, hint, L.ptr(out), L.ptr(radii), ctypes.byref(state), L.stream(), None)
    torch.cuda.synchronize()
    return (out,), int(state.n_isects)


def _surfel(x, hint):
    from gspl_amd import _lib as L
    from gspl_amd.ops import _frame
    state = L.SurfelState()
    out, allmap = torch.empty(3, H, W, device=DEV), torch.empty(7, H, W, device=DEV)
    radii = torch.empty(N, dtype=torch.int32, device=DEV)
    scales2 = x["scales"][:, :2].contiguous()
    with _frame.FrameBlocks(DEV) as frame:
        L.call("gspl_rasterize_surfel_fwd", N, 3, 16, L.ptr(x["means"]), L.ptr(scales2), L.ptr(x["quats"]), L.ptr(x["shs"]), None, L.ptr(x["opac"]),
               L.ptr(x["view"]), L.ptr(x["proj"]), L.ptr(x["campos"]), L.ptr(x["bg"]), W, H, 1.0, frame.callback, None, L.ptr(out), L.ptr(allmap),
               L.ptr(radii), ctypes.byref(state), L.stream())
    torch.cuda.synchronize()
    return (out, allmap), int(state.n_isects)


def _refusals(monkeypatch, run, x, hint, expect_tags):
    """One good frame, then every call-back position refused in turn, each followed by another good frame."""
    from gspl_amd import _lib as L
    from gspl_amd.ops import _frame
    plain = _frame.allocate
    tags = []
    refuse_at = [None]

    def allocate(nbytes, device, tag):
        tags.append(tag)
        if len(tags) - 1 == refuse_at[0]:
            raise MemoryError(f"block {refuse_at[0]} refused")
        return plain(nbytes, device, tag)

    monkeypatch.setattr(_frame, "allocate", allocate)
    good, n_isects = run(x, hint)
    good_tags = list(tags)
    print(f"hint {hint}: n_isects {n_isects}, call-backs {good_tags}")
    assert good_tags == expect_tags
    optional = (L.GSPL_BUF_PACKED, L.GSPL_BUF_CHECKPOINTS)
    for k, tag in enumerate(good_tags):
        del tags[:]
        refuse_at[0] = k
        if tag in optional:      # the library does without the block
            got, n = run(x, hint)
            assert n == n_isects and all(torch.equal(a, b) for a, b in zip(got, good)), f"hint {hint}: frame without block {k} (tag {tag}) differs"
        else:
            with pytest.raises(MemoryError, match=f"block {k} refused"):
                run(x, hint)
        assert tags[:k + 1] == good_tags[:k + 1]
        torch.cuda.synchronize()      # the refused call left the stream healthy
        del tags[:]
        refuse_at[0] = None
        again, n = run(x, hint)
        assert tags == good_tags and n == n_isects, f"hint {hint}: the frame after refusal {k} took another path"
        assert all(torch.equal(a, b) for a, b in zip(again, good)), f"hint {hint}: the frame after refusal {k} differs from the first"
    return n_isects


def test_inria_forward_refused_blocks_in_every_list_regime(monkeypatch):
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib as L
    x = _inputs()
    G, I, P, B, LW, LI, C = (L.GSPL_BUF_GEOMETRY, L.GSPL_BUF_IMAGE, L.GSPL_BUF_PACKED, L.GSPL_BUF_BINNING, L.GSPL_BUF_LISTS_WORK,
                             L.GSPL_BUF_LISTS, L.GSPL_BUF_CHECKPOINTS)
    # no hint: the host reads the list length, then builds the lists
    n_isects = _refusals(monkeypatch, _inria, x, 0, [G, I, P, B, LW, LI, C])
    assert n_isects > 256      # (more than one segment: the checkpoint block is asked for)
    # a hint that holds: the lists are built speculatively, nothing is redone
    assert _refusals(monkeypatch, _inria, x, n_isects + 64, [G, I, P, B, LW, LI, C]) == n_isects
    # too low a hint (16 entries: no checkpoint block for it): the lists are redone with the real length
    assert _refusals(monkeypatch, _inria, x, 16, [G, I, P, B, LW, LI, LW, LI, C]) == n_isects


def test_surfel_forward_refused_blocks(monkeypatch):
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib as L
    n_isects = _refusals(monkeypatch, _surfel, _inputs(), 0,
                         [L.GSPL_BUF_GEOMETRY, L.GSPL_BUF_IMAGE, L.GSPL_BUF_BINNING, L.GSPL_BUF_LISTS_WORK, L.GSPL_BUF_LISTS])
    assert n_isects > 0

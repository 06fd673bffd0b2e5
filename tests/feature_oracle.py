"""fp64 reference for wide-feature compositing (tests only): `O.composite_fwd` / `O.composite_bwd` of oracle/gsplat_oracle.py,
run in slices of channels.

The C oracle keeps at most 16 channels per pixel, so wider inputs go through it 16 channels at a time and the slices are
concatenated.  That is exact: the blending weights, `last_ids` and the fragile map do not depend on the channels — which is
asserted, slice against slice."""
import numpy as np

from oracle import gsplat_oracle as O

ORACLE_MAX_D = 16


def _slices(D, width=ORACLE_MAX_D):
    return [slice(s, min(D, s + width)) for s in range(0, D, width)]


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def feature_fwd(mode, means2d, conics, features, opacities, background, W, H, offsets, flatten_ids, tile=16, width=ORACLE_MAX_D):
    """-> (out [H,W,D] f64, alpha [H,W] f64, last_ids [H,W] i32, fragile [H,W] u8)."""
    features = _np(features)
    background = None if background is None else _np(background)
    outs, maps = [], None
    for sl in _slices(features.shape[1], width):
        out, alpha, last, frag = O.composite_fwd(mode, means2d, conics, features[:, sl], opacities,
                                                 None if background is None else background[sl], W, H, offsets, flatten_ids, tile=tile)
        if maps is None:
            maps = (alpha, last, frag)
        else:
            assert np.array_equal(alpha, maps[0]) and np.array_equal(last, maps[1]) and np.array_equal(frag, maps[2]), \
                "the oracle's alpha / last_ids / fragile maps depend on the channel slice"
        outs.append(out)
    return (np.concatenate(outs, axis=-1),) + maps


def feature_bwd(mode, means2d, conics, features, opacities, background, W, H, offsets, flatten_ids, out_alphas, last_ids, v_out,
                fragile_px=None, tile=16, width=ORACLE_MAX_D):
    """-> v_features [N,D] f64: the oracle's `v_colors`, slice by slice (v_out [H,W,D]; no upstream gradient of alpha)."""
    features, v_out = _np(features), _np(v_out)
    background = None if background is None else _np(background)
    grads = []
    for sl in _slices(features.shape[1], width):
        ref = O.composite_bwd(mode, means2d, conics, features[:, sl], opacities, None if background is None else background[sl], W, H,
                              offsets, flatten_ids, out_alphas, last_ids, np.ascontiguousarray(v_out[..., sl]), None,
                              fragile_px=fragile_px, tile=tile)
        grads.append(ref["v_colors"])
    return np.concatenate(grads, axis=1)

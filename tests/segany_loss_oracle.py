"""fp64 oracle of the SegAnyGS training step behind the renderer (include/gspl_hip.h section 24), written from the section's formulas.
tests/test_segany_loss_cpu.py pins it to the reference's own run (tests/golden/ref_segany_loss.npz); tests/test_segany_loss.py pins the
kernels to it.

Every sum comes with the sum of the absolute terms it is made of (`*_abs`).  A pair is FRAGILE when at some scale its correlation lies
within 2 (C + 8) eps32 of 0.75, of 0.5 or of 0: there a float32 run may decide the hard-sample test (or, at 0, the relu's slope) the
other way.  `loss(..., lock=selected)` takes the selection of the fragile pairs from a given byte map (the locked-parity pattern); the
relu's slope cannot be locked that way, so the terms of the pairs fragile at 0 are returned on their own (`*_fragile`) and belong into
the tolerance of the gradients they feed."""
import functools
import os

import numpy as np
import torch

from spotless_oracle import EPS32, resample_axis

F32 = np.float32


# ---- stage 1 -------------------------------------------------------------------------------------------------------------------------
def mask_stats(masks):
    """masks [N, H, W] -> area [N] int64, cover [H, W] int64, mean_size [H, W] float64, and the float32 bound of mean_size: the
    numerator's one rounding and the division's (2 roundings, eps32 has the factor 2 of room), plus the 1e-9 the float32 sum loses."""
    m = np.asarray(masks) != 0
    area = m.reshape(m.shape[0], -1).sum(axis=1).astype(np.int64)
    cover = m.sum(axis=0).astype(np.int64)
    numerator = np.tensordot(area, m.astype(np.int64), axes=1)
    mean_size = numerator / (cover + 1e-9)
    return area, cover, mean_size, (2 * EPS32 + 1e-9) * mean_size


def mean_size_f32(masks):
    """mean_size as float32 arithmetic gives it from the exact numerator (below 2^24 in the tests' frames): what the reference's float32
    sums leave, and what the pair weight is formed from."""
    area, cover, _, _ = mask_stats(masks)
    numerator = np.tensordot(area, (np.asarray(masks) != 0).astype(np.int64), axes=1)
    assert numerator.max() < 2 ** 24
    return (numerator.astype(F32) / (cover.astype(F32) + F32(1e-9))).astype(F32)


def membership(masks, order, pixel_index):
    """-> member [S, N] bool (column i = the i-th mask in `order`), words [S, ceil(N / 64)] int64 (bit i of word w = column 64 w + i)."""
    m = np.asarray(masks) != 0
    N = m.shape[0]
    member = m.reshape(N, -1)[np.asarray(order)][:, np.asarray(pixel_index)].T
    NW = (N + 63) // 64
    padded = np.zeros((member.shape[0], 64 * NW), dtype=np.uint64)
    padded[:, :N] = member
    words = (padded.reshape(-1, NW, 64) << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)
    return member, words.view(np.int64)


# ---- stage 2 -------------------------------------------------------------------------------------------------------------------------
def pair_labels(member, scale_index, upper):
    """The closed form: -> gt [Ns, S, S] bool, labels [S, S] uint16 (bit n = gt[n]), counts [3] (none, all, the rest; full matrix)."""
    member = np.asarray(member, dtype=bool)
    S, N = member.shape
    index = np.arange(N)
    gt = []
    for si, up in zip(np.asarray(scale_index).tolist(), np.asarray(upper).tolist()):
        if up:
            common = member.astype(np.int64) @ member.T.astype(np.int64)
            gt.append(common > 0)
            continue
        big = member & (index <= si)
        head = np.where(big.any(axis=1), N - 1 - np.argmax(big[:, ::-1], axis=1), -1)
        small = (member & (index > si)).astype(np.int64)
        gt.append(((head[:, None] == head[None, :]) & (head[:, None] >= 0)) | ((small @ small.T) > 0))
    gt = np.stack(gt)
    labels = (gt.astype(np.uint32) << np.arange(len(gt), dtype=np.uint32)[:, None, None]).sum(axis=0).astype(np.uint16)
    total = gt.sum(axis=0)
    counts = np.array([(total == 0).sum(), (total == len(gt)).sum(), ((total != 0) & (total != len(gt))).sum()], dtype=np.int64)
    return gt, labels, counts


def unpack_labels(labels, Ns):
    return ((np.asarray(labels).astype(np.uint32)[None] >> np.arange(Ns, dtype=np.uint32)[:, None, None]) & 1).astype(bool)


# ---- stage 3 -------------------------------------------------------------------------------------------------------------------------
def pair_weight(a):
    """The pair weight [S, S] in float32, every operation rounded on its own in the section's order."""
    a = np.asarray(a, dtype=F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        P = F32(a.max() * a.max())
        R = np.maximum(F32(P / F32(a.min() * a.min())), F32(1))
        q = np.maximum((P / (a[:, None] * a[None, :]).astype(F32)).astype(F32), F32(1))
        unit = ((q - F32(1)).astype(F32) / F32(R - F32(1))).astype(F32)
        return ((unit * F32(9)).astype(F32) + F32(1)).astype(F32)


def sample_taps(Hr, Wr, mask_hw, pixel_index, dtype=np.float32):
    """-> taps [4, S] flat texel indices and weights [4, S]: the bilinear sample at the centre of each mask pixel, indices and weights
    formed in float32 as the kernels form them (they carry no error of their own)."""
    mh, mw = mask_hw
    p = np.asarray(pixel_index, dtype=np.int64)
    i, j = p // mw, p % mw
    y0, y1, yl, yh = (t[i] for t in resample_axis(Hr, mh, dtype))
    x0, x1, xl, xh = (t[j] for t in resample_axis(Wr, mw, dtype))
    taps = np.stack([y0 * Wr + x0, y0 * Wr + x1, y1 * Wr + x0, y1 * Wr + x1])
    return taps, np.stack([yh * xh, yh * xl, yl * xh, yl * xl])


def thresholds(counts):
    with np.errstate(divide="ignore", invalid="ignore"):
        half = F32(F32(counts[2]) / F32(2))
        return F32(half / F32(counts[1])), F32(half / F32(counts[0]))


def _adjoint_abs(K, X, norm, F, gates, taps, weights, shape):
    """The absolute sums behind the gradients for non-negative pair coefficients K [Ns, S, S] (symmetric)."""
    C = F.shape[1]
    dX = np.einsum("nhj,njc->nhc", K, np.abs(X))
    dot = (np.abs(X) * dX).sum(axis=2, keepdims=True)
    dU = (dX + np.abs(X) * dot) / np.maximum(norm, 1e-12)
    v_F = (dU * np.abs(gates)[:, None, :]).sum(axis=0)
    v_gates = (dU * np.abs(F)[None]).sum(axis=1)
    v_rendered = np.zeros((C, shape[1] * shape[2]))
    for t, w in zip(taps, weights):
        np.add.at(v_rendered.T, t, v_F * w[:, None])
    return v_F, v_gates, v_rendered.reshape(shape)


def loss(rendered, mask_hw, pixel_index, gates, labels, counts, a, rand, lock=None, grad_out=1.0, dtype=np.float32):
    """`dtype`: the precision the resampling's indices and weights are formed in (float32 as the kernels, float64 as the reference's
    float64 run).  -> dict: F, F_abs [S, C]; kappa (the largest ||F_abs g|| / ||F g||: how much the sample's rounding is amplified in X);
    corr [Ns, S, S]; weight [S, S] float32; own [S, S] uint8 the oracle's own selection (bit 0 M+, bit 1 M-; h < j); selected: the one
    used (own, with the fragile pairs taken from `lock`); fragile [S, S] bool (h < j); n_pos, n_neg; loss, cosine_pos, cosine_neg;
    loss_abs (the selected weights' share with |corr| counted as 1); v_rendered, v_gates, v_F with *_abs and *_fragile."""
    rendered = np.asarray(rendered, dtype=np.float64)
    gates_np = np.asarray(gates, dtype=np.float64)
    C, Hr, Wr = rendered.shape
    Ns, S = gates_np.shape[0], len(pixel_index)
    taps, weights = sample_taps(Hr, Wr, mask_hw, pixel_index, dtype)
    r_t = torch.from_numpy(rendered).requires_grad_(True)
    g_t = torch.from_numpy(gates_np).requires_grad_(True)
    flat = r_t.reshape(C, -1)
    F_t = sum(flat[:, torch.from_numpy(t)] * torch.from_numpy(w) for t, w in zip(taps, weights)).t()      # [S, C]
    F_t.retain_grad()
    F_abs = sum(np.abs(rendered).reshape(C, -1)[:, t] * w for t, w in zip(taps, weights)).T
    U = F_t[None] * g_t[:, None, :]
    norm_t = U.norm(dim=2, keepdim=True)
    X_t = U / norm_t.clamp_min(1e-12)
    corr_t = torch.einsum("nhc,njc->nhj", X_t, X_t)
    corr = corr_t.detach().numpy()
    F, X, norm = F_t.detach().numpy(), X_t.detach().numpy(), norm_t.detach().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.linalg.norm(F_abs[None] * np.abs(gates_np)[:, None, :], axis=2) / norm[:, :, 0]
    kappa = float(np.nanmax(np.where(norm[:, :, 0] > 0, ratio, 1.0)))

    gt = unpack_labels(labels, Ns)
    total = gt.sum(axis=0)
    upper_tri = np.triu(np.ones((S, S), dtype=bool), 1)
    band = 2 * (C + 8) * EPS32
    near = lambda value: (np.abs(corr - value) <= band).any(axis=0)
    fragile_zero = (np.abs(corr) <= band) & upper_tri[None]
    fragile = (near(0.75) | near(0.5) | near(0.0)) & upper_tri
    t_pos, t_neg = thresholds(counts)
    rnd = np.asarray(rand, dtype=F32)
    inconsistent = (total != 0) & (total != Ns)
    with np.errstate(invalid="ignore"):
        in_pos = ((total == Ns) & (rnd < t_pos)) | ((corr < 0.75) & gt).any(axis=0) | inconsistent
        in_neg = ((total == 0) & (rnd < t_neg)) | ((corr > 0.5) & ~gt).any(axis=0) | inconsistent
    own = ((in_pos & upper_tri).astype(np.uint8) | ((in_neg & upper_tri).astype(np.uint8) << 1))
    selected = own if lock is None else np.where(fragile, np.asarray(lock, dtype=np.uint8), own)
    m_pos, m_neg = (selected & 1).astype(bool), (selected & 2).astype(bool)
    n_pos, n_neg = int(m_pos.sum()), int(m_neg.sum())
    weight = pair_weight(a)
    w_t = torch.from_numpy(weight.astype(np.float64))
    gt_t = torch.from_numpy(gt.astype(np.float64))
    pos_terms = (w_t * (gt_t * corr_t).sum(dim=0))[torch.from_numpy(m_pos)]
    neg_terms = (w_t * ((1 - gt_t) * torch.relu(corr_t)).sum(dim=0))[torch.from_numpy(m_neg)]
    value = -pos_terms.sum() / (Ns * torch.tensor(float(n_pos))) + neg_terms.sum() / (Ns * torch.tensor(float(n_neg)))
    finite = bool(torch.isfinite(value))
    if finite:
        (value * grad_out).backward()
    zero = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        w64 = weight.astype(np.float64)
        share_pos = np.where(m_pos, w64, 0.0) / (Ns * n_pos) if n_pos else np.zeros((S, S))
        share_neg = np.where(m_neg, w64, 0.0) / (Ns * n_neg) if n_neg else np.zeros((S, S))
        loss_abs = float((share_pos * gt.sum(axis=0)).sum() + (share_neg * (~gt).sum(axis=0)).sum())
        full = np.concatenate([corr[:, upper_tri], corr[:, upper_tri], corr[:, np.eye(S, dtype=bool)]], axis=1)
        full_gt = np.concatenate([gt[:, upper_tri], gt[:, upper_tri], gt[:, np.eye(S, dtype=bool)]], axis=1)
        cosine_pos = full[full_gt].sum() / full_gt.sum() if full_gt.any() else np.nan
        cosine_neg = full[~full_gt].sum() / (~full_gt).sum() if (~full_gt).any() else np.nan
    out = dict(F=F, F_abs=F_abs, kappa=kappa, corr=corr, weight=weight, own=own, selected=selected, fragile=fragile, n_pos=n_pos, n_neg=n_neg,
               loss=float(value.detach()), loss_abs=loss_abs, cosine_pos=float(cosine_pos), cosine_neg=float(cosine_neg),
               v_rendered=zero(r_t), v_gates=zero(g_t), v_F=zero(F_t))
    # the coefficients' absolute values, mirrored to both triangles: all of them, and those of the pairs fragile at 0 as if active
    scale = abs(float(grad_out))
    K = scale * (share_pos[None] * gt + share_neg[None] * (~gt & (corr > 0)))
    K_fragile = scale * (share_neg[None] * (~gt & fragile_zero))
    shape = (C, Hr, Wr)
    for name, k in (("abs", K), ("fragile", K_fragile)):
        k = np.nan_to_num(k + k.transpose(0, 2, 1))
        v_F, v_gates, v_rendered = _adjoint_abs(k, X, norm, F, gates_np, taps, weights, shape)
        out["v_F_" + name], out["v_gates_" + name], out["v_rendered_" + name] = v_F, v_gates, v_rendered
    out["texel_sharing"] = int(np.bincount(taps.reshape(-1)).max())
    return out


# ---- seeded inputs shared by the CPU and the GPU tests --------------------------------------------------------------------------------
def recipe_features(name, count, C, rng):
    """The two feature recipes: "randn", and "centres" = 12 randn centres + 0.35 randn (about 8 % of the pairs then exceed 0.75, so
    both hard-sample branches fire both ways)."""
    if name == "randn":
        return rng.standard_normal((count, C))
    centres = rng.standard_normal((12, C))
    return centres[rng.integers(0, 12, size=count)] + 0.35 * rng.standard_normal((count, C))


def scale_picks(N, Ns, rng):
    """scale_index [Ns] as the reference forms it (-1 in front, N - 1 behind, index 0 among the picks when there is room) and the
    upper flags: the scale in front, and the largest scale where it was picked."""
    picks = [int(v) for v in rng.permutation(N)[:max(Ns - 2, 0)]]
    if Ns >= 3 and 0 not in picks:
        picks[0] = 0
    index = np.array([-1] + picks + [N - 1], dtype=np.int32)[:Ns]
    upper = np.array([1] + [1 if v == 0 and k % 2 else 0 for k, v in enumerate(index[1:])], dtype=np.uint8)
    return index, upper


def make_case(S, C, Ns, recipe="randn", seed=0, N=20, mask_hw=None, render_hw=None, density=0.25):
    """Everything stage 3 reads, seeded: a rendered map of recipe features (at the mask's size unless `render_hw` says otherwise: the
    sampled features are then the recipe's own rows), S sampled pixels in raster order, random memberships with at least one mask per
    pixel and their labels, mean sizes in 5 .. 500, the [S, S] draw and sigmoid(randn) gates."""
    rng = np.random.default_rng(seed)
    if mask_hw is None:
        mw = int(np.ceil(np.sqrt(S))) + 1
        mask_hw = (-(-S // mw) + 1, mw)
    render_hw = render_hw or mask_hw
    rendered = recipe_features(recipe, render_hw[0] * render_hw[1], C, rng).T.reshape(C, *render_hw).astype(F32)
    pixel_index = np.sort(rng.choice(mask_hw[0] * mask_hw[1], size=S, replace=False)).astype(np.int32)
    member = rng.random((S, N)) < density
    member[np.arange(S), rng.integers(0, N, size=S)] = True
    scale_index, upper = scale_picks(N, Ns, rng)
    gt, labels, counts = pair_labels(member, scale_index, upper)
    return dict(rendered=rendered, mask_hw=tuple(mask_hw), pixel_index=pixel_index, gates=(1 / (1 + np.exp(-rng.standard_normal((Ns, C))))).astype(F32),
                labels=labels, counts=counts.astype(np.int32), a=rng.uniform(5, 500, size=S).astype(F32), rand=rng.random((S, S), dtype=F32),
                member=member, scale_index=scale_index, upper=upper)


def loss_of(case, **kw):
    return loss(case["rendered"], case["mask_hw"], case["pixel_index"], case["gates"], case["labels"], case["counts"], case["a"], case["rand"], **kw)


def random_masks(N, H, W, seed):
    """N rectangles of mixed sizes (uint8) with a few uncovered pixels, and scales that grow with the area (distinct)."""
    rng = np.random.default_rng(seed)
    masks = np.zeros((N, H, W), dtype=np.uint8)
    for i in range(N):
        h, w = rng.integers(1, H + 1), rng.integers(1, W + 1)
        y, x = rng.integers(0, H - h + 1), rng.integers(0, W - w + 1)
        masks[i, y:y + h, x:x + w] = 1
    scales = (np.sqrt(masks.reshape(N, -1).sum(axis=1)) * rng.uniform(0.9, 1.1, size=N) + 1e-3 * np.arange(N)).astype(F32)
    return masks, scales


# ---- the reference's recorded frame (tests/golden/ref_segany_loss.npz) ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_segany_loss.npz")))


@functools.lru_cache(maxsize=None)
def golden_inputs():
    """The inputs of the three stages as the reference formed them from the recorded draws."""
    g = golden()
    scales, N = g["mask_scales"], len(g["mask_scales"])
    order = np.argsort(-scales, kind="stable")
    sorted_scales = scales[order]
    scale_index = np.concatenate([[-1], g["draw_randperm"][:8], [N - 1]]).astype(np.int32)
    ub = np.float32(g["upper_bound_scale"])
    front = np.float32(ub + np.float32(ub * g["draw_rand1"][0]))
    upper = np.concatenate([[front >= ub], sorted_scales[scale_index[1:]] >= ub]).astype(np.uint8)
    pixel_index = np.flatnonzero(g["sampled_ray"].reshape(-1)).astype(np.int32)
    member, words = membership(g["masks"], order, pixel_index)
    return dict(order=order, scale_index=scale_index, upper=upper, pixel_index=pixel_index, member=member, words=words,
                a=mean_size_f32(g["masks"]).reshape(-1)[pixel_index])

"""CPU oracles for `ops.knn_points` and `ops.smooth_features`.

K nearest neighbours: fp64 brute force with a stable sort, i.e. ordered by (d^2, index) — the tie rule of the HIP kernel — and a
k-d tree (scipy) as the independent cross-check of the sorted distances.  Where fewer than K reference points exist the trailing
entries are zeros, as pytorch3d publishes.

Smoothing: the reference's formula (internal/segany_splatting.py:280-308) restated in fp64 torch, autograd for the gradient:
    n = F.normalize(x, dim=-1, p=2);  m = n[idx[:, columns]].mean(1);  out = m / (|m| + 1e-9)
"""
import numpy as np
import torch


def knn_brute(queries, refs, K):
    """-> (d2 [P1, K] fp64 ascending, idx [P1, K] int64), ties by the lower index, zero padding behind min(K, P2)."""
    q, r = np.asarray(queries, dtype=np.float64), np.asarray(refs, dtype=np.float64)
    P1, P2 = q.shape[0], r.shape[0]
    d2 = np.zeros((P1, K))
    idx = np.zeros((P1, K), dtype=np.int64)
    n = min(K, P2)
    if P1 == 0 or n == 0:
        return d2, idx
    for s in range(0, P1, 512):
        block = ((q[s:s + 512, None, :] - r[None, :, :]) ** 2).sum(-1)
        order = np.argsort(block, axis=1, kind="stable")[:, :n]
        idx[s:s + 512, :n] = order
        d2[s:s + 512, :n] = np.take_along_axis(block, order, axis=1)
    return d2, idx


def knn_kdtree_d2(queries, refs, K):
    """Sorted squared distances [P1, min(K, P2)] from scipy's k-d tree (fp64)."""
    from scipy.spatial import cKDTree
    q, r = np.asarray(queries, dtype=np.float64), np.asarray(refs, dtype=np.float64)
    n = min(K, r.shape[0])
    d, _ = cKDTree(r).query(q, k=n)
    return (d.reshape(q.shape[0], n)) ** 2


def smooth_reference(features, idx, columns=None, dtype=torch.float64):
    """The reference's arithmetic on `features` (a leaf that may require grad), `idx` [N, K] int64, `columns` a list or None."""
    x = features.to(dtype)
    n = torch.nn.functional.normalize(x, dim=-1, p=2)
    sel = idx if columns is None else idx[:, torch.as_tensor(columns, dtype=torch.long, device=idx.device)]
    m = n[sel, :].mean(dim=1)
    return m / (m.norm(dim=-1, keepdim=True) + 1e-9)


def smooth_reference_with_grad(features_np, idx_np, weights_np, columns=None):
    """-> (out [N, D] fp64, d(sum(out * weights)) / d features [N, D] fp64), numpy in and out."""
    x = torch.from_numpy(np.asarray(features_np, dtype=np.float64)).requires_grad_(True)
    out = smooth_reference(x, torch.from_numpy(np.asarray(idx_np, dtype=np.int64)), columns)
    (out * torch.from_numpy(np.asarray(weights_np, dtype=np.float64))).sum().backward()
    return out.detach().numpy(), x.grad.numpy()

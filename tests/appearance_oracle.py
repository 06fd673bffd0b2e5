"""Oracle of the fused appearance MLP (include/gspl_hip.h section 21): explicit forward AND backward formulas on the CPU, in float64 or,
for integer-valued data, in int64.  Nothing here uses autograd; tests/test_appearance_shims.py checks these formulas against autograd
on a torch.nn restatement.

    x_n   = [f^_n | e^ | enc(d_n)]           f^ = f / max(|f|, eps), e^ = e / max(|e|, eps) with `normalize`, else f and e
    z_0   = W_0[:, :F] f^ + W_0[:, F+E:] enc + b_0',   b_0' = b_0 + W_0[:, F:F+E] e^        (the embedding folded into the bias)
    a_l   = relu(z_l);   z_l = W_l a_(l-1) + b_l;   out = act(z_last);   rows the mask drops: out = 0 and no contribution anywhere

    delta_last = v_out * act'(z_last);   v_W_l = delta_l^T a_(l-1);   v_b_l = sum_n delta_l;   delta_(l-1) = (delta_l W_l) * [a_(l-1) > 0]
    v_W_0[:, :F] = delta_0^T f^;  v_W_0[:, F+E:] = delta_0^T enc;  v_W_0[:, F:F+E] = v_b_0 (x) e^;  v_e^ = W_0[:, F:F+E]^T v_b_0
    v_f^ = delta_0 W_0[:, :F];    normalize backward: v_x = (v_x^ - x^ <x^, v_x^>) / |x| where |x| >= eps, v_x^ / eps below it
The direction d = (mean - camera_center) / max(|.|, 1e-12) is a constant (detached in the reference)."""
from __future__ import annotations

import torch

EPS = 1e-12
EXACT_LIMIT = 2 ** 24


def view_encoding(d: torch.Tensor, n_frequencies: int) -> torch.Tensor:
    """x, sin(2^0 x), cos(2^0 x), sin(2^1 x), ... (internal/encodings/positional_encoding.py:35-40)."""
    parts = [d]
    for k in range(n_frequencies):
        parts += [torch.sin(d * 2.0 ** k), torch.cos(d * 2.0 ** k)]
    return torch.cat(parts, dim=-1)


class _Bound:
    """max over every product of sum |a| |b|: below 2^24, fp32 holds every partial sum of integer data exactly, in ANY order."""

    def __init__(self):
        self.value = 0

    def mm(self, a, b):
        if not a.dtype.is_floating_point and a.numel() and b.numel():
            self.value = max(self.value, int((a.abs().double() @ b.abs().double()).max()))      # (exact: far below 2^53)
        return a @ b

    def see(self, t):
        if not t.dtype.is_floating_point and t.numel():
            self.value = max(self.value, int(t.abs().max()))
        return t


def _normalize(x):
    norm = x.norm(dim=-1, keepdim=True)
    return x / norm.clamp_min(EPS), norm


def _normalize_backward(v_hat, x_hat, norm):
    inside = (v_hat - x_hat * (x_hat * v_hat).sum(-1, keepdim=True)) / norm.clamp_min(EPS)
    return torch.where(norm >= EPS, inside, v_hat / EPS)


def forward(features, weights, biases, embedding, mask=None, means=None, camera_center=None, n_view_frequencies=0, normalize=False,
            output_activation="sigmoid", dtype=torch.float64):
    """-> (out [N, n_out], cache).  dtype int64: integer data, `normalize` and the encoding off, activation "none"."""
    exact = dtype == torch.int64
    assert not exact or (not normalize and n_view_frequencies == 0 and output_activation == "none")
    cpu = lambda t: t.detach().cpu().to(dtype)
    f, e = cpu(features), cpu(embedding).reshape(-1)
    ws, bs = [cpu(w) for w in weights], [cpu(b) for b in biases]
    N, F = f.shape
    E = e.numel()
    keep = torch.ones(N, dtype=torch.bool) if mask is None else mask.detach().cpu().bool()
    bound = _Bound()
    f_norm = e_norm = None
    f_hat, e_hat = f[keep], e
    if normalize:
        f_hat, f_norm = _normalize(f_hat)
        e_hat, e_norm = _normalize(e_hat)
    enc = None
    if n_view_frequencies > 0:
        d = cpu(means)[keep] - cpu(camera_center).reshape(1, 3)
        d = d / d.norm(dim=-1, keepdim=True).clamp_min(EPS)
        enc = view_encoding(d, n_view_frequencies)
    w0 = ws[0]
    folded = bs[0] + bound.mm(w0[:, F:F + E], e_hat.reshape(-1, 1)).reshape(-1)
    z = bound.mm(f_hat, w0[:, :F].T) + folded
    if enc is not None:
        z = z + enc @ w0[:, F + E:].T
    acts = []
    for w, b in zip(ws[1:], bs[1:]):
        acts.append(bound.see(z.clamp_min(0)))
        z = bound.mm(acts[-1], w.T) + b
    bound.see(z)
    y = torch.sigmoid(z) if output_activation == "sigmoid" else z
    out = torch.zeros((N, ws[-1].shape[0]), dtype=dtype)
    out[keep] = y
    cache = dict(keep=keep, f_hat=f_hat, f_norm=f_norm, e_hat=e_hat, e_norm=e_norm, enc=enc, acts=acts, y=y, ws=ws, F=F, E=E, N=N,
                 normalize=normalize, sigmoid=output_activation == "sigmoid", bound=bound, dtype=dtype)
    return out, cache


def backward(cache, v_out):
    """-> dict(v_features [N, F], v_weights [..], v_biases [..], v_embedding [E]); masked rows of v_features are zeros."""
    c = cache
    bound, ws, F, E, keep = c["bound"], c["ws"], c["F"], c["E"], c["keep"]
    delta = v_out.detach().cpu().to(c["dtype"])[keep]
    if c["sigmoid"]:
        delta = delta * c["y"] * (1 - c["y"])
    v_ws, v_bs = [None] * len(ws), [None] * len(ws)
    for layer in range(len(ws) - 1, 0, -1):
        a = c["acts"][layer - 1]
        v_ws[layer] = bound.mm(delta.T, a)
        v_bs[layer] = bound.see(delta.sum(0))
        bound.mm(delta.abs().T, torch.ones_like(delta[:, :1]))
        delta = bound.mm(delta, ws[layer]) * (a > 0).to(delta.dtype)
    v_b0 = bound.see(delta.sum(0))
    bound.mm(delta.abs().T, torch.ones_like(delta[:, :1]))
    v_w0 = torch.zeros_like(ws[0])
    v_w0[:, :F] = bound.mm(delta.T, c["f_hat"])
    v_w0[:, F:F + E] = bound.see(v_b0.reshape(-1, 1) * c["e_hat"].reshape(1, -1))
    if c["enc"] is not None:
        v_w0[:, F + E:] = delta.T @ c["enc"]
    v_ws[0], v_bs[0] = v_w0, v_b0
    v_e = bound.mm(ws[0][:, F:F + E].T, v_b0.reshape(-1, 1)).reshape(-1)
    v_f = bound.mm(delta, ws[0][:, :F])
    if c["normalize"]:
        v_f = _normalize_backward(v_f, c["f_hat"], c["f_norm"])
        v_e = _normalize_backward(v_e, c["e_hat"], c["e_norm"])
    v_features = torch.zeros((c["N"], F), dtype=c["dtype"])
    v_features[keep] = v_f
    return dict(v_features=v_features, v_weights=v_ws, v_biases=v_bs, v_embedding=v_e)


def exact(features, weights, biases, embedding, v_out, mask=None):
    """Integer data in int64 -> (out, gradients, bound); asserts that every intermediate, and the sum of absolute products behind
    every element of every matrix product, stays below 2^24, so exact fp32 arithmetic must reproduce these bits in any order."""
    out, cache = forward(features, weights, biases, embedding, mask=mask, output_activation="none", dtype=torch.int64)
    grads = backward(cache, v_out)
    bound = cache["bound"].value
    assert bound < EXACT_LIMIT, f"integer test data leaves the exact range of fp32: {bound} >= 2^24"
    return out, grads, bound


def integer_case(N, F, E, H, n_layers, n_out, seed=0, amplitude=None):
    """Integer-valued float32 test data with asymmetric weights: (features, weights, biases, embedding, v_out).  Amplitude 3 for small
    N, 1 from 1024 rows on (the weight gradients sum over the rows)."""
    g = torch.Generator().manual_seed(seed)
    amp = amplitude if amplitude is not None else (3 if N < 1024 else 1)
    draw = lambda *shape, a=amp: torch.randint(-a, a + 1, shape, generator=g).float()
    features = draw(N, F)
    weights, biases, fan_in = [], [], F + E
    for layer in range(n_layers):
        rows = n_out if layer == n_layers - 1 else H
        w = draw(rows, fan_in)
        w[0, -1] += 1          # never symmetric, never the identity
        weights.append(w)
        biases.append(draw(rows))
        fan_in = H
    return features, weights, biases, draw(E), draw(N, n_out, a=min(amp, 2))

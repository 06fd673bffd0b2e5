"""`ops.mip_filter_3d` and `ops.mip_apply_3d_filter` (include/gspl_hip.h section 28, csrc/mip.hip) on the GPU against the fp64 oracle
tests/mip_oracle.py, which tests/test_mip.py pins to the reference's own run.

Error bounds, in unit roundoffs u = 2^-24.

Filter.  Rows whose decision margin (tests/mip_oracle.py) is below 1e-4 may be decided either way in float32 and are skipped; at most
1 % of a case's rows may be such.  On the others `valid_any` is equal and |distance - oracle| <= 5 u z_scale (tests/test_mip.py has
the derivation: a three-term fmaf chain plus T).  `filter_3d` is then compared BIT FOR BIT with the reference's two final float32
operations evaluated by torch on the op's own distance and valid_any: that pins the fill, the maximum and the two roundings without
depending on an undecided row.

Apply, the kernel's formula: s = exp(x) for raw scales (HIP's expf: 2 ulp = 4 u allowed, d_s = 4 u; else d_s = 0), o = 1 / (1 + exp(-y))
for raw opacities (exp 4 u, the sum 1 u, the quotient 1 u: d_o = 6 u; else 0); b = s s + f f (positive terms: 2 u + 2 d_s),
out = sqrt(b) (1 u + half of b's, and d ln out / d ln s <= 1): d_s + 3 u; r = s / out: d_s + 4 u; coef = r_0 r_1 r_2:
3 d_s + 14 u; o coef: d_o + 3 d_s + 15 u.  So
    scales_out  K = 3 + 4 raw_s              second  K = 15 + 12 raw_s + 6 raw_o          (relative, plus K 2^-126 for underflow)
Gradient of the scales: g_i = v_out_i r_i + v_coef (r_j r_k) f^2 / (out_i b_i), times s_i for raw scales, with v_coef = v o: the first
term d_s + 5 u, the second (d_o + u) + (2 d_s + 9 u) + (3 d_s + 8 u) + 2 u, the sum 1 u, the chain d_s + u:
    g_scales    K = 22 + 24 raw_s + 6 raw_o  of `mag_scales` = |v_out_i| r_i + |v_coef| r_j r_k f^2 / (out_i b_i) (times s_i)
Gradient of the opacities: v coef (K = 16 + 12 raw_s), times o (1 - o) for raw opacities, where 1 - o carries d_o o absolute:
    g_opacities |v| coef ((K + 2 + d_o) o (1 - o) + d_o o o) for raw opacities, K |v| coef otherwise."""
import numpy as np
import pytest
import torch

import mip_oracle as MO
from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = MO.U
MARGIN, FRAGILE_CAP = 1e-4, 0.01
TINY = 2.0 ** -126


@pytest.fixture(scope="module")
def ref():
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_mip.npz")) as z:
        return {k: z[k] for k in z.files}


def blind_camera():
    """p.z = -y - 50: every point of the fixture (y >= -1.5) is behind it"""
    row = np.zeros(16, dtype=np.float32)
    row[:9] = np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0]], dtype=np.float32).reshape(-1)
    row[9:12] = [40.0, 0.0, -50.0]
    row[12:16] = [450.0, 450.0, 320.0, 240.0]
    return row


def extra_cameras(n, seed):
    g = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        a, height = g.uniform(0, 2 * np.pi), g.uniform(-1, 1)
        position = np.array([4 * np.cos(a), height, 4 * np.sin(a)])
        forward = -position / np.linalg.norm(position)
        right = np.cross(forward, [0.0, -1.0, 0.0])
        right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(forward, right), forward])
        rows.append(np.concatenate([R.reshape(-1), -R @ position, [300.0 + 3 * i, 310.0, 320.0, 200.0]]))
    return np.asarray(rows, dtype=np.float32)


def case_table(ref, C):
    table = ref["table"]
    if C == 1:
        return table[3:4]
    if C == 2:
        return np.stack([table[10], blind_camera()])
    if C == 12:
        return table
    return np.concatenate([table, blind_camera()[None], extra_cameras(C - 13, seed=1)])


def case_means(ref, N):
    """the whole fixture, or its first rows with one in eight taken from the rows no camera sees"""
    if N > 4096:
        return ref["means"]
    k = N // 8
    return np.ascontiguousarray(np.concatenate([ref["means"][:N - k], ref["means"][4096:4096 + k]]))


FILTER_CASES = [(N, C) for N in (1, 63, 64, 65, 257, 4160) for C in (1, 2, 12)] + [(257, 70)]


@pytest.mark.parametrize("N,C", FILTER_CASES)
def test_filter_against_the_oracle(ref, N, C):
    from gspl_amd import ops
    means, table = case_means(ref, N), case_table(ref, C)
    assert means.shape == (N, 3) and table.shape == (C, 16)
    o = MO.filter(means, table)
    firm = o["margin"] >= MARGIN
    print(f"N {N} C {C}: {int((~firm).sum())} undecided rows, {int(o['valid_any'].sum())} valid, seen per camera {o['seen'].tolist()[:14]}")
    assert (~firm).sum() <= FRAGILE_CAP * N
    if C in (2, 70):
        assert o["seen"][1 if C == 2 else 12] == 0          # the camera that sees nothing
    m, t = torch.from_numpy(means).to(DEV), torch.from_numpy(table).to(DEV)
    filt, distance, valid = ops.mip_filter_3d(m, t, return_parts=True)
    assert tuple(filt.shape) == (N, 1) and tuple(distance.shape) == (N,) and valid.dtype == torch.bool
    got_valid, got_distance = valid.cpu().numpy(), distance.cpu().numpy().astype(np.float64)
    assert np.array_equal(got_valid[firm], o["valid_any"][firm])
    err = np.abs(got_distance - o["distance"])[firm]
    print(f"  distance: worst error / (u z_scale) = {(err / (U * o['z_scale'][firm])).max() if err.size else 0:.3f} (bound 5)")
    assert (err <= 5 * U * o["z_scale"][firm]).all()
    # the fill, the maximum and the two final roundings, on the op's own parts
    want = MO.filter_from_parts(distance, valid, t[:, 12].max().clamp(min=0.))
    assert torch.equal(filt[:, 0], want)
    # identical bits between runs, with and without the optional outputs, and into the caller's buffer
    buf = torch.empty(N, 1, device=DEV)
    assert ops.mip_filter_3d(m, t, out=buf) is buf and torch.equal(buf, filt)
    again = ops.mip_filter_3d(m, t, return_parts=True)
    assert all(torch.equal(a, b) for a, b in zip(again, (filt, distance, valid)))


def test_filter_with_no_valid_row_keeps_the_initial_distance(ref):
    from gspl_amd import ops
    m, t = torch.from_numpy(ref["means"][4096:]).to(DEV), torch.from_numpy(ref["table"]).to(DEV)
    filt, distance, valid = ops.mip_filter_3d(m, t, return_parts=True)
    assert not bool(valid.any()) and bool((distance == 100000.0).all())
    assert torch.equal(filt[:, 0], torch.full_like(distance, 100000.0) / t[:, 12].max() * (0.2 ** 0.5))


def test_filter_refusals_on_the_device():
    from gspl_amd import ops
    m, t = torch.zeros(5, 3, device=DEV), torch.zeros(2, 16, device=DEV)
    with pytest.raises(RuntimeError, match="camera_table is on cpu"):
        ops.mip_filter_3d(m, t.cpu())
    with pytest.raises(ValueError, match="out must be"):
        ops.mip_filter_3d(m, t, out=torch.empty(5, 1))
    with pytest.raises(ValueError, match="at least one camera"):
        ops.mip_filter_3d(m, t[:0])


# ---- apply ----------------------------------------------------------------------------------------------------------------------------
def apply_inputs(N, raw_s, raw_o, seed=0):
    g = torch.Generator().manual_seed(100 + N + seed)
    x = torch.randn(N, 3, generator=g) - 4                     # log-scales: s = 0.002 .. 0.15
    y = 2 * torch.randn(N, 1, generator=g)                     # logits: o = 0.003 .. 0.997
    f = 0.001 + 0.05 * torch.rand(N, 1, generator=g)
    vs, vo = torch.randn(N, 3, generator=g), torch.randn(N, generator=g)
    return (x if raw_s else torch.exp(x)), (y if raw_o else torch.sigmoid(y)), f, vs, vo


def check_apply(scales, opacities, f, vs, vo, raw_s, raw_o, compensation):
    from gspl_amd import ops
    N = scales.shape[0]
    o = MO.apply(scales.numpy(), f.numpy(), None if opacities is None else opacities.numpy(), raw_s, raw_o, compensation, vs.numpy(), vo.numpy())
    s_leaf = scales.to(DEV).requires_grad_(True)
    o_leaf = None if opacities is None else opacities.to(DEV).requires_grad_(True)
    new_s, second = ops.mip_apply_3d_filter(s_leaf, f.to(DEV), o_leaf, raw_scales=raw_s, raw_opacities=raw_o, opacity_compensation=compensation)
    loss = (new_s * vs.to(DEV)).sum()
    if second is not None:
        assert second.shape == ((N,) if opacities is None else opacities.shape)
        loss = loss + (second.reshape(N) * vo.to(DEV)).sum()
    loss.backward()
    ds, do = 4 * raw_s, 6 * raw_o
    np64 = lambda t: t.detach().cpu().numpy().astype(np.float64)

    def within(name, got, want, k, mag=None):
        bound = k * U * (np.abs(want) if mag is None else mag) + k * TINY
        worst = (np.abs(got - want) / bound).max()
        print(f"  {name}: worst error / bound = {worst:.3f} (K = {k})")
        assert worst <= 1.0, name

    within("scales_out", np64(new_s), o["scales_out"], 3 + ds)
    within("g_scales", np64(s_leaf.grad), o["g_scales"], 22 + 6 * ds + do, o["mag_scales"])
    if o["second"] is None:
        assert second is None
        return new_s, second
    k_second = (15 + 3 * ds + do) if compensation else max(do, 1)
    within("second", np64(second).reshape(N), o["second"], k_second)
    if opacities is not None:
        v, coef = np.abs(o["v_second"]), (o["coef"] if compensation else np.ones(N))
        k_c = (16 + 3 * ds) if compensation else 1
        if raw_o:
            mag = v * coef * ((k_c + 2 + do) * o["o"] * (1 - o["o"]) + do * o["o"] * o["o"])
            within("g_opacities", np64(o_leaf.grad).reshape(N), o["g_opacities"], 1, mag)
        else:
            within("g_opacities", np64(o_leaf.grad).reshape(N), o["g_opacities"], k_c, v * coef)
    return new_s, second


@pytest.mark.parametrize("N", [1, 64, 65, 4099])
@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
@pytest.mark.parametrize("mode", ["opacities", "coef", "no_compensation"])
def test_apply_against_the_oracle(N, raw, mode):
    scales, opacities, f, vs, vo = apply_inputs(N, raw, raw)
    print(f"N {N} raw {raw} {mode}")
    if mode == "coef":
        check_apply(scales, None, f, vs, vo, raw, False, True)
    else:
        check_apply(scales, opacities, f, vs, vo, raw, raw, mode == "opacities")
        if mode == "no_compensation":
            check_apply(scales, None, f, vs, vo, raw, False, False)          # the scales alone: no second output


def test_apply_on_the_golden_inputs(ref):
    """The same fixture on which tests/test_mip.py ties the oracle to the reference's float32 values."""
    t = lambda k: torch.from_numpy(ref[k])
    new_s, second = check_apply(t("a_scales"), t("a_opacities"), t("a_filter"), t("a_vs"), t("a_vo"), False, False, True)
    # ... and next to the reference's own float32 values: both sit within their bounds of the oracle, so within the sum of each other
    assert np.abs(new_s.detach().cpu().numpy() - ref["on1_scales"]).max() <= (3 + 3) * U * ref["on1_scales"].max()
    assert np.abs(second.detach().cpu().numpy() - ref["on1_opacities"]).max() <= (15 + 10) * U * ref["on1_opacities"].max()


def test_apply_degenerate_rows_stay_finite():
    """Raw scales of -50 (s = 2e-22: s^2 is below float32's range, the reference's det1 is zero and its gradient NaN) and a row with
    filter_3d = 0: outputs and gradients are finite, coef is exactly 1 and the scales pass unchanged where f = 0."""
    from gspl_amd import ops
    x = torch.full((6, 3), -4.0)
    x[0], x[1], x[2, 1] = -50.0, -50.0, -50.0
    f = torch.full((6, 1), 0.01)
    f[1], f[3] = 0.0, 0.0
    y = torch.zeros(6, 1)
    for opacities in (y, None):
        s_leaf = x.to(DEV).requires_grad_(True)
        o_leaf = None if opacities is None else opacities.to(DEV).requires_grad_(True)
        new_s, second = ops.mip_apply_3d_filter(s_leaf, f.to(DEV), o_leaf, raw_scales=True, raw_opacities=opacities is not None)
        (new_s.sum() + second.sum()).backward()
        tensors = [new_s, second, s_leaf.grad] + ([] if o_leaf is None else [o_leaf.grad])
        assert all(bool(torch.isfinite(t).all()) for t in tensors)
        coef = second.reshape(-1) if opacities is None else second.reshape(-1) / 0.5
        ordinary = (1.0 + (0.01 / np.exp(-4.0)) ** 2) ** -1.5          # (s / sqrt(s^2 + f^2))^3 of the rows left alone
        assert coef[1].item() == 1.0 and coef[3].item() == 1.0 and 0.0 <= coef[0].item() < 1e-30
        assert abs(coef[4].item() - ordinary) <= 40 * U * ordinary and abs(coef[5].item() - ordinary) <= 40 * U * ordinary
        for row in (1, 3):          # out = s exactly, d out / d raw = s and no coefficient term (s by float64's exp: the kernel's expf has 2 ulp)
            s64 = torch.exp(x[row].double())
            assert float(((new_s[row].detach().cpu().double() - s64).abs() / s64).max()) <= 4 * U
            assert torch.equal(s_leaf.grad[row], new_s[row].detach())
    a = torch.rand(9, 3, device=DEV).requires_grad_(True)
    new_s, coef = ops.mip_apply_3d_filter(a, torch.zeros(9, device=DEV))
    assert torch.equal(new_s, a) and bool((coef == 1.0).all())


def test_apply_launches_alone_and_their_buffers():
    from gspl_amd import ops
    scales, opacities, f, vs, vo = (t.to(DEV) for t in apply_inputs(65, True, True))
    want_s, want_o = ops.mip_apply_3d_filter_forward(scales, f, opacities, raw_scales=True, raw_opacities=True)
    bs, bo = torch.empty(65, 3, device=DEV), torch.empty(65, device=DEV)
    got = ops.mip_apply_3d_filter_forward(scales, f, opacities, raw_scales=True, raw_opacities=True, scales_out=bs, opacities_out=bo)
    assert got[0] is bs and got[1] is bo and torch.equal(bs, want_s) and torch.equal(bo, want_o) and tuple(want_o.shape) == (65,)
    g1 = ops.mip_apply_3d_filter_backward(scales, f, opacities, vs, vo, raw_scales=True, raw_opacities=True)
    g2 = ops.mip_apply_3d_filter_backward(scales, f, opacities, vs, vo, raw_scales=True, raw_opacities=True, v_scales=torch.empty_like(bs),
                                          v_opacities=torch.empty_like(bo))
    assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])
    assert ops.mip_apply_3d_filter_backward(scales, f, opacities, vs, None, raw_scales=True, raw_opacities=True, want_opacities=False)[1] is None
    with pytest.raises(ValueError, match="scales_out must be"):
        ops.mip_apply_3d_filter_forward(scales, f, opacities, scales_out=torch.empty(65, 4, device=DEV))
    with pytest.raises(ValueError, match="opacities_out must be"):
        ops.mip_apply_3d_filter_forward(scales, f, opacities, opacities_out=torch.empty(65, 1, device="cpu"))
    with pytest.raises(ValueError, match="nothing to write"):
        ops.mip_apply_3d_filter_forward(scales, f, None, opacity_compensation=False, opacities_out=bo)
    with pytest.raises(RuntimeError, match="opacities is on cpu"):
        ops.mip_apply_3d_filter(scales, f, opacities.cpu())

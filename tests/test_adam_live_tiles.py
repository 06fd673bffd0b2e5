"""`selective_adam_kernel`'s skipping form at the sizes where a mapping of rows to lanes, waves and workgroups can go wrong.  The file
was written for a live-tile form of the kernel (a workgroup gathers the live 16-byte chunks of a tile of R = 64 rows), which measured no
faster and is kept only as tools/experiments/adam_live_tiles/ — hence the name and R.  The cases do not depend on the form.  What they
check in the tree (csrc/adam.hip): tensors of 32 or more floats per row pass over no-op chunks one by one, narrower tensors decide per
group of 8 lanes (128 bytes: if one chunk of the group is live, all 8 take the dense update), both in one launch.  "Last row of the
first tile" and "first row of the second tile" are here simply single live rows: in a narrow tensor one live group among dead ones.  No
case runs a tensor past the 16 384-workgroup cap of an unlimited launch; `max_blocks` = 1 and 3 run the same grid stride.
The contract is BIT equality with the dense update — the same library with `GSPL_ADAM_SKIP_NOOP=0`, which the native code reads
once: parameters and both moments as int32 views, `torch.equal`.

As in tests/test_adam_noop_rows.py the dense results come from ONE child process (this file run as a script with the switch off) that
computes every case from the same seeds and saves them; the tests compute the cases in this process and compare.

Shapes: N in {1, 3, 4, R - 1, R, R + 1, 2 R + 2, 1000} rows; one launch holds rows of
45 (the model's), 48, 33 and 32 floats (chunk by chunk) and 1, 3 and 4 (group by group): N * 45 is odd or no multiple of 4 for
most N.  Per N every combination of
  liveness   none / all / every other row / only the last row of the first tile / only the first row of the second tile / every fifth
             row (dead neighbours on both sides: the 16-byte chunks at its ends straddle a live and a dead row);
  grad_rows  absent / present — then also SET for rows whose gradient is all zero and CLEAR for rows that have live moments;
  visible    absent / all ones / masking every third live row / masking every dead row (the dead half of a straddling chunk);
over two steps: the second step's gradient rows are the first's moved on by one, so dead rows become live and live rows are left with
moments and a zero gradient.  Dead rows hold -0.0, denormals, inf and NaN in `p`; some carry moments of -0.0, which is no no-op (the
dense update turns them into +0.0).  `max_blocks` = 1 and 3: one workgroup strides over the whole tensor."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SWITCH = "GSPL_ADAM_SKIP_NOOP"
R = 64                                                   # rows per tile of the live-tile form
SIZES = (1, 3, 4, R - 1, R, R + 1, 2 * R + 2, 1000)
WIDTHS = (45, 1, 48, 3, 33, 4, 32)
LRS = (1.25e-4, 5e-2, 2.5e-3, 1.6e-4, 5e-3, 1e-3, 2e-3)
PATTERNS = ("none", "all", "alternate", "last-of-tile", "first-of-next-tile", "fifth")
VISIBLE = ("absent", "ones", "mask-live", "mask-dead")
ODD = (-0.0, 1e-41, float("inf"), float("nan"), -1e-39, float("-inf"))


def _dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().clone()


def _pattern(name, n):
    r = torch.arange(n)
    if name == "none":
        return torch.zeros(n, dtype=torch.bool)
    if name == "all":
        return torch.ones(n, dtype=torch.bool)
    if name == "alternate":
        return r % 2 == 0
    if name == "last-of-tile":
        return r == min(R, n) - 1
    if name == "first-of-next-tile":
        return r == (R if n > R else 0)
    return r % 5 == 2


def _launch(L, items, n, vis, rows, step, max_blocks=0):
    table = (L.AdamTensor * len(items))()
    for k, (p, g, m, v, lr, w) in enumerate(items):
        table[k] = L.AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), lr, w)
    L.call("gspl_selective_adam_rows", len(items), table, n, L.ptr(vis), L.ptr(rows), 0.9, 0.999, 1e-15, 1 - 0.9 ** step, (1 - 0.999 ** step) ** 0.5,
           int(max_blocks), L.stream())


def _combo(n, pattern, vis_mode, use_rows, max_blocks=0, snapshots=(1, 2)):
    """Two launches over the seven tensors; {f"{width}/{name}@{step}": int32 bits}, and the state before the first as `@0`."""
    from gspl_amd import _lib as L
    g = torch.Generator().manual_seed(1000 * n + 10 * PATTERNS.index(pattern) + VISIBLE.index(vis_mode))
    base = _pattern(pattern, n)
    rows_idx = torch.arange(n)
    special = pattern not in ("none", "all")
    neg_moments = special & (rows_idx % 11 == 5) & ~base                        # moments of -0.0, never a gradient
    old_moments = special & (rows_idx % 13 == 7) & ~base & ~neg_moments         # live moments from before, no gradient: its flag stays clear
    odd_p = ~base & (rows_idx % 2 == 1)
    if vis_mode == "absent":
        vis = None
    elif vis_mode == "ones":
        vis = torch.ones(n, dtype=torch.uint8)
    elif vis_mode == "mask-live":
        live_rows = base.nonzero().flatten()
        vis = torch.ones(n, dtype=torch.uint8)
        vis[live_rows[::3]] = 0
    else:
        vis = base.to(torch.uint8)
    odd = torch.tensor(ODD)
    state = []
    for w in WIDTHS:
        p = torch.randn(n, w, generator=g)
        m, v = torch.zeros(n, w), torch.zeros(n, w)
        rr = odd_p.nonzero().flatten()
        p[rr] = odd[(torch.arange(w)[None, :] + rr[:, None]) % len(odd)]
        rr = neg_moments.nonzero().flatten()
        which = (torch.arange(w)[None, :] + rr[:, None]) % 3                    # m alone, v alone, both
        m[rr] = torch.where(which != 1, -0.0, 0.0)
        v[rr] = torch.where(which != 0, -0.0, 0.0)
        k = int(old_moments.sum())
        m[old_moments] = 0.1 * torch.randn(k, w, generator=g)
        v[old_moments] = 0.01 * torch.rand(k, w, generator=g)
        state.append([t.to(_dev()) for t in (p, m, v)])
    out = {}
    for (p, m, v), w in zip(state, WIDTHS):
        out.update({f"{w}/p@0": _bits(p), f"{w}/m@0": _bits(m), f"{w}/v@0": _bits(v)})
    dev_vis = vis.to(_dev()) if vis is not None else None
    for step in (1, 2):
        has = base if step == 1 or not special else torch.roll(base, 1)
        grads = []
        for w in WIDTHS:
            gr = torch.zeros(n, w)
            gr[has] = torch.randn(int(has.sum()), w, generator=g)
            grads.append(gr.to(_dev()))
        flagged = has | (special & (rows_idx % 7 == 3) & ~old_moments)          # some rows are flagged over a gradient of zeros
        rows = flagged.to(torch.uint8).to(_dev()) if use_rows else None
        _launch(L, [(p, gr, m, v, lr, w) for (p, m, v), gr, lr, w in zip(state, grads, LRS, WIDTHS)], n, dev_vis, rows, step, max_blocks)
        if step in snapshots:
            for (p, m, v), w in zip(state, WIDTHS):
                out.update({f"{w}/p@{step}": _bits(p), f"{w}/m@{step}": _bits(m), f"{w}/v@{step}": _bits(v)})
    out["vis"] = vis.clone() if vis is not None else torch.ones(n, dtype=torch.uint8)
    out["base"] = base.clone()
    return out


def _combos(n):
    # (the largest size keeps the second step alone and half of the visibility modes: what it adds is many tiles per launch)
    vis_modes = VISIBLE if n < 1000 else ("absent", "mask-dead")
    return [(pattern, vis_mode, use_rows) for pattern in PATTERNS for vis_mode in vis_modes for use_rows in (False, True)]


def _size(n):
    snaps = (1, 2) if n < 1000 else (2,)
    return {f"{pattern}/{vis_mode}/rows{int(use_rows)}": _combo(n, pattern, vis_mode, use_rows, snapshots=snaps)
            for pattern, vis_mode, use_rows in _combos(n)}


@pytest.fixture(scope="module")
def dense(tmp_path_factory):
    """{N: {combination: its result}} from a process in which the library never skips a chunk."""
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert os.environ.get(SWITCH, "1") != "0", f"{SWITCH}=0: this process would compare the dense update with itself"
    path = str(tmp_path_factory.mktemp("adam_dense_tiles") / "dense.pt")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, **{SWITCH: "0"}), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(path)


def _same(got, ref, what):
    assert sorted(got) == sorted(ref)
    for k in got:
        assert torch.equal(got[k], ref[k]), f"{what}: {k} differs from the dense update in {int((got[k] != ref[k]).sum())} of {got[k].numel()} words"


def _untouched_where_invisible(res, what):
    """An invisible row keeps the bits of p, m and v — the dead half of a straddling chunk among them."""
    hidden = res["vis"] == 0
    for w in WIDTHS:
        for name in "pmv":
            first, last = res[f"{w}/{name}@0"].view(-1, w), res[f"{w}/{name}@2"].view(-1, w)
            assert torch.equal(first[hidden], last[hidden]), f"{what}: {w}/{name} moved in an invisible row"


@pytest.mark.parametrize("n", SIZES)
def test_bits_equal_the_dense_update(dense, n):
    got = _size(n)
    assert sorted(got) == sorted(dense[n])
    for combo, res in got.items():
        _same(res, dense[n][combo], f"N = {n}, {combo}")
        _untouched_where_invisible(res, f"N = {n}, {combo}")
    # the cases hold what they are meant to hold
    for w in (45, 32):
        v_none = got["none/absent/rows1"][f"{w}/v@2"]
        assert not bool(v_none.any()), "no row is live: no moment moves"
        assert torch.equal(got["none/absent/rows1"][f"{w}/p@0"], got["none/absent/rows1"][f"{w}/p@2"])
        assert bool((got["all/absent/rows1"][f"{w}/v@2"] != 0).all())
    if n >= 16:
        res = got["fifth/absent/rows1"]
        v = res["45/v@2"].view(n, 45)
        assert bool((v == 0).all(dim=1).any()) and bool((v != 0).all(dim=1).any())
        became_live = torch.roll(res["base"], 1) & ~res["base"]
        assert bool((v[became_live] != 0).all()), "rows without a gradient in the first step have one in the second"
        assert bool((res["45/m@0"] == -2 ** 31).any()) and not bool((res["45/m@2"] == -2 ** 31).any()), "moments of -0.0 become +0.0"
        p = res["45/p@2"].view(torch.float32)
        assert bool(torch.isnan(p).any()) and bool(torch.isinf(p).any())


@pytest.mark.parametrize("max_blocks", [1, 3])
@pytest.mark.parametrize("n", [2 * R + 2, 1000])
def test_one_workgroup_strides_over_several_tiles(dense, n, max_blocks):
    """The dense update does not depend on the grid: the reference is the one of the unlimited launch."""
    for pattern, vis_mode, use_rows in _combos(n):
        if vis_mode not in ("absent", "mask-dead"):
            continue
        got = _combo(n, pattern, vis_mode, use_rows, max_blocks=max_blocks, snapshots=(1, 2) if n < 1000 else (2,))
        _same(got, dense[n][f"{pattern}/{vis_mode}/rows{int(use_rows)}"], f"N = {n}, max_blocks = {max_blocks}, {pattern}/{vis_mode}/rows{int(use_rows)}")


if __name__ == "__main__":
    assert os.environ.get(SWITCH) == "0"
    sys.path.insert(0, ROOT)
    import gspl_amd  # noqa: F401
    torch.save({n: _size(n) for n in SIZES}, sys.argv[1])

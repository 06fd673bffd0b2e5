"""The 3DGS-MCMC route without a GPU: the fp64 oracle against closed forms and published known answers, the plugin's configuration
against the reference's, the `gsplat` stand-in still refusing `gsplat.relocation`, and one relocation + growth event of the reference's
own controller next to `gspl_amd.mcmc`'s, both on the oracle (tests/mcmc_reference_worker.py, in a process of its own)."""
import ast
import dataclasses
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mcmc_oracle as MO

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = os.environ.get("GSPL_REFERENCE_ROOT", "/root/reference")
REF_CONTROLLER = os.path.join(REF_ROOT, "internal", "density_controllers", "mcmc_density_controller.py")
needs_reference = pytest.mark.skipif(not os.path.exists(REF_CONTROLLER), reason="reference tree not present")


def test_relocation_oracle_closed_forms():
    o = np.array([0.005, 0.3, 0.7, 0.999])
    s = np.array([[1e-3, 1.0, 1e3]] * 4)
    new_o, new_s, kappa = MO.relocation(o, s, np.ones(4, dtype=np.int64))
    assert np.allclose(new_o, o, rtol=1e-14) and np.allclose(new_s, s, rtol=1e-14) and np.allclose(kappa, 1.0)
    new_o, new_s, _ = MO.relocation(o, s, np.full(4, 2))
    x = 1 - np.sqrt(1 - o)
    assert np.allclose(new_o, x, rtol=1e-14)
    assert np.allclose(new_s, (o / (2 * x - x * x / math.sqrt(2)))[:, None] * s, rtol=1e-13)
    # clamping: 0 -> 1, beyond n_max -> n_max
    a = MO.relocation(o, s, np.array([0, -3, 60, 51]), n_max=51)
    b = MO.relocation(o, s, np.array([1, 1, 51, 51]), n_max=51)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_relocation_preserves_the_opacity_of_the_stack():
    # Eq. 9's purpose: n copies of opacity x composite to the old opacity, 1 - (1 - x)^n = o
    o = np.geomspace(0.005, 0.99, 17)
    for n in (2, 5, 51):
        new_o, _, kappa = MO.relocation(o, np.ones((17, 3)), np.full(17, n))
        assert np.allclose(1 - (1 - new_o) ** n, o, rtol=1e-12) and np.all(kappa >= 1)


def test_philox_known_answers():
    # Random123's known-answer vectors of philox4x32-10 (kat_vectors): zero, all-ones and pi digits
    f = 0xFFFFFFFF
    cases = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((f, f, f, f), (f, f), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in cases:
        got = MO.philox4x32_10(*([c] for c in ctr), *key)[0]
        assert tuple(int(v) for v in got) == want
    # curand_init(seed, subsequence = i, offset)'s first block: offset / 4 in counter words 0-1, the row in words 2-3
    b = MO.mcmc_bits(3, seed=(7 << 32) | 5, offset=(2 << 34) | 12, first=(1 << 32) + 4)
    ref = MO.philox4x32_10([3] * 3, [2] * 3, [4, 5, 6], [1, 1, 1], 5, 7)
    assert np.array_equal(b, ref)
    u = MO.uniforms(np.array([[0, 0xFFFFFFFF, 255, 256]], dtype=np.uint32))
    assert u[0, 0] == 2.0 ** -24 and u[0, 1] == 1.0 and u[0, 2] == 2.0 ** -24 and u[0, 3] == 2.0 ** -23


def test_perturbation_oracle():
    rng = np.random.default_rng(1)
    n = 50
    means, s, eps = rng.normal(size=(n, 3)), np.exp(rng.normal(-3, 0.5, size=(n, 3))), rng.normal(size=(n, 3))
    q = rng.normal(size=(n, 4))
    o = rng.uniform(0, 1, size=n)
    qn = q / np.linalg.norm(q, axis=1, keepdims=True)
    got = MO.perturb(means, s, qn, o, eps, 80.0, raw=False)
    R = MO.rotation_matrix(qn)
    for i in range(n):
        cov = R[i] @ np.diag(s[i] ** 2) @ R[i].T
        c = 80.0 / (1 + math.exp(-100 * ((1 - o[i]) - 0.995)))
        assert np.allclose(got[i], means[i] + c * cov @ eps[i], rtol=1e-12, atol=1e-15)
    raw = MO.perturb(means, np.log(s), 2.5 * q, np.log(o / (1 - o)), eps, 80.0, raw=True)
    assert np.allclose(raw, got, rtol=1e-10, atol=1e-14)


def test_regulariser_oracle_gradients_by_finite_differences():
    rng = np.random.default_rng(2)
    o, s = rng.normal(size=(6, 1)), rng.normal(size=(6, 3))
    for raw in (True, False):
        go, gs = MO.reg_bwd(o, s, 0.3, 0.7, raw)
        h = 1e-6
        for idx in ((0, 0), (4, 0)):
            d = np.zeros_like(o)
            d[idx] = h
            fd = (sum(MO.reg_fwd(o + d, s, 0.3, 0.7, raw)) - sum(MO.reg_fwd(o - d, s, 0.3, 0.7, raw))) / (2 * h)
            assert abs(fd - go[idx]) < 1e-8
        for idx in ((1, 2), (5, 0)):
            d = np.zeros_like(s)
            d[idx] = h
            fd = (sum(MO.reg_fwd(o, s + d, 0.3, 0.7, raw)) - sum(MO.reg_fwd(o, s - d, 0.3, 0.7, raw))) / (2 * h)
            assert abs(fd - gs[idx]) < 1e-8


def test_ops_refuse_cpu_tensors():
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.compute_relocation(torch.ones(3), torch.ones(3, 3), torch.ones(3, dtype=torch.int32), torch.ones(4, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.perturb_means_(torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 4), torch.zeros(2), raw=True, noise_scale=1.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.mcmc_regularization(torch.zeros(2, 1), torch.zeros(2, 3), 0.1, 0.1, raw=True)


def test_relocation_stays_unregistered_in_the_gsplat_stand_in():
    import gspl_amd  # noqa: F401
    import gspl_amd.renderers  # noqa: F401
    import gspl_amd.mcmc  # noqa: F401
    from gspl_amd import compat
    compat.install()
    with pytest.raises(ImportError):
        from gsplat.relocation import compute_relocation  # noqa: F401


def _reference_fields():
    tree = ast.parse(open(REF_CONTROLLER).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "MCMCDensityController")
    out = {}
    for st in cls.body:
        if isinstance(st, ast.AnnAssign) and isinstance(st.target, ast.Name):
            out[st.target.id] = ast.literal_eval(st.value) if st.value is not None else dataclasses.MISSING
    return out


@needs_reference
def test_plugin_fields_and_defaults_equal_the_reference():
    import gspl_amd  # noqa: F401
    from gspl_amd.mcmc import HipMCMCDensityController
    ours = {f.name: f.default for f in dataclasses.fields(HipMCMCDensityController)}
    ref = _reference_fields()
    assert list(ours) == list(ref) and ours == ref
    assert ours["noise_lr"] == 5e5 and ours["N_max"] == 51 and ours["cap_max"] is dataclasses.MISSING
    with pytest.raises(AssertionError):
        HipMCMCDensityController(cap_max=0).instantiate()


@needs_reference
def test_reference_controller_and_plugin_relocate_identically():
    r = subprocess.run([sys.executable, os.path.join(HERE, "mcmc_reference_worker.py"), REF_ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["dead"] > 0 and d["n_sampled"] == [d["dead"], d["n"] - d["n0"]] and d["n"] == int(1.05 * d["n0"])
    names = d["property_names"]
    for variant in ("plugin", "standalone"):
        v = d[variant]
        assert v["n"] == d["n"] and v["indices_equal"], variant
        assert v["params_equal"] == names and v["moments_equal"] == names, variant
    assert d["touched_rows_zeroed"] and d["other_rows_kept"]

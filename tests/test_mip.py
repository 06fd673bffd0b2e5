"""The Mip-Splatting route without a GPU: the fp64 oracle tests/mip_oracle.py against the reference's own float32 run
(tests/golden/ref_mip.npz, made by tests/golden/make_mip_golden.py from the unedited `MipSplattingUtils`), the CPU restatements of
`ops.mip_filter_3d` / `ops.mip_apply_3d_filter` and the stand-ins of `gspl_amd.mip` against the same file bit for bit, the reference's
unedited model method and renderer mixins next to the plugin's (tests/mip_reference_worker.py, a process of its own; skipped without the
reference tree), the configs, the checkpoint round trip and every refusal of the ops that needs no device.

Error bounds, in unit roundoffs u = 2^-24 (float32):
  distance   p.z is a three-term dot product plus T (any order, with or without fma: at most 4 roundings on terms whose absolute sum is
             S = |R_2| . |x| + |T_2|), so |p.z - exact| <= 4 u S (1 + O(u)); max(., 0.001) and the minimum over the cameras are exact
             selections, so the bound of a row is 5 u x the largest S over the cameras (`z_scale`; 5 for 4 and the O(u^2) terms).
  filter_3d  two more roundings (the quotient and the product; sqrt(0.2) is the same float32 on both sides): relative
             5 u z_scale / distance + 3 u.  A filled row (no camera sees it) carries the error of the maximum, at most 5 u max z_scale."""
import dataclasses
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import mip_oracle as MO

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_mip.npz")
REF_ROOT = os.environ.get("GSPL_REFERENCE_ROOT", "/root/reference")
needs_reference = pytest.mark.skipif(not os.path.exists(os.path.join(REF_ROOT, "internal", "models", "mip_splatting.py")),
                                     reason="the reference tree is not present")
U = MO.U
MARGIN, FRAGILE_CAP, HIDDEN_FLOOR = 1e-4, 0.01, 0.01
N_SEEN = 4096


@pytest.fixture(scope="module")
def ref():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def oracle(ref):
    return MO.filter(ref["means"], ref["table"])


@pytest.fixture(scope="module")
def worker():
    r = subprocess.run([sys.executable, os.path.join(HERE, "mip_reference_worker.py"), REF_ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def cameras_of(table):
    return [types.SimpleNamespace(R=r[:9].reshape(3, 3), T=r[9:12], fx=r[12], fy=r[13], width=r[14].to(torch.int32), height=r[15].to(torch.int32))
            for r in torch.as_tensor(table)]


# ---- the oracle and the fixture -------------------------------------------------------------------------------------------------------
def test_oracle_matches_the_reference_run(ref, oracle):
    """Every validity flag equal (the reference's float32 run decides no row differently from float64 on this fixture), distances and
    filter within the bounds of the module docstring."""
    assert np.array_equal(oracle["valid_any"], ref["valid_any"])
    d_err = np.abs(oracle["distance"] - ref["distance"])
    print(f"distance: worst error / (u z_scale) = {(d_err / (U * oracle['z_scale'])).max():.3f} (bound 5)")
    assert (d_err <= 5 * U * oracle["z_scale"]).all()
    filled = np.where(oracle["valid_any"], oracle["distance"], oracle["fill"])
    scale = np.where(oracle["valid_any"], oracle["z_scale"], oracle["z_scale"].max())
    bound = (5 * U * scale / filled + 3 * U) * oracle["filter"]
    f_err = np.abs(oracle["filter"] - ref["filter"][:, 0])
    print(f"filter_3d: worst error / bound = {(f_err / bound).max():.3f}")
    assert ref["filter"].shape == (ref["means"].shape[0], 1) and (f_err <= bound).all()


def test_the_fixture_has_few_undecided_rows_and_enough_invisible_ones(ref, oracle):
    """Conditions on the fixture, not tolerances: at most 1 % of the rows within 1e-4 of a threshold (those a float32 run may decide
    either way; the GPU tests skip them and assert the same cap), at least 1 % that no camera sees (they exercise the fill), every
    camera sees something, and the two image sizes and rising fx are there."""
    near = oracle["margin"] < MARGIN
    hidden = ~oracle["valid_any"]
    print(f"{int(near.sum())} of {near.size} rows with a margin below {MARGIN}; {int(hidden.sum())} invisible; seen per camera {oracle['seen'].tolist()}")
    assert near.mean() <= FRAGILE_CAP and hidden.mean() >= HIDDEN_FLOOR
    assert not hidden[:N_SEEN].any() and hidden[N_SEEN:].all() and (oracle["seen"] > 0).all()
    table = ref["table"]
    assert table.shape == (12, 16) and len({tuple(r) for r in table[:, 14:16]}) == 2 and (np.diff(table[:, 12]) > 0).all()
    assert oracle["max_fx"] == table[-1, 12] and oracle["fill"] == oracle["distance"][~hidden].max()


def test_the_reference_filter_is_the_two_operation_expression(ref):
    d, v = torch.from_numpy(ref["distance"]), torch.from_numpy(ref["valid_any"])
    got = MO.filter_from_parts(d, v, torch.from_numpy(ref["table"])[:, 12].max())
    assert torch.equal(got[:, None], torch.from_numpy(ref["filter"]))


APPLY_CASES = [("on1", True, True), ("on0", False, True), ("sc", True, False)]


@pytest.mark.parametrize("key,compensation,with_opacities", APPLY_CASES)
def test_apply_oracle_matches_the_reference_run(ref, key, compensation, with_opacities):
    """The reference's float32 values within K u of the fp64 oracle: scales_out 3 u (square, add, sqrt on positive terms, the square
    root halving what it gets); coef 9 u (det1 5 u, det2 8 u, the quotient 1, halved by the root, + 1 for the root; 9 for 8);
    o coef 10 u; the gradients 24 u of `mag_scales_ref`, the sum of the absolute terms of autograd's expression (its two terms in
    d coef / d s cancel; each is a product of at most 24 rounded factors), the opacities' (v coef) 10 u."""
    o = MO.apply(ref["a_scales"], ref["a_filter"], ref["a_opacities"] if with_opacities else None, compensation=compensation,
                 v_scales=ref["a_vs"], v_second=ref["a_vo"])
    within = lambda got, want, k, mag=None: (np.abs(got - want) <= k * U * (np.abs(want) if mag is None else mag)).all()
    assert within(ref[key + "_scales"], o["scales_out"], 3)
    assert within(ref[key + "_g_scales"], o["g_scales"], 24, o["mag_scales_ref"])
    if with_opacities:
        assert within(ref[key + "_opacities"][:, 0], o["second"], 10)
        assert within(ref[key + "_g_opacities"][:, 0], o["g_opacities"], 10)
    else:
        assert within(ref[key + "_coef"], o["second"], 9)


# ---- the CPU restatements, bit for bit ------------------------------------------------------------------------------------------------
def test_cpu_filter_is_the_reference_bit_for_bit(ref):
    from gspl_amd import mip, ops
    means, table = torch.from_numpy(ref["means"]), torch.from_numpy(ref["table"])
    filt, distance, valid = ops.mip_filter_3d(means, table, return_parts=True)
    assert filt.dtype == torch.float32 and tuple(filt.shape) == (means.shape[0], 1) and valid.dtype == torch.bool
    assert np.array_equal(filt.numpy(), ref["filter"]) and np.array_equal(distance.numpy(), ref["distance"]) and np.array_equal(valid.numpy(), ref["valid_any"])
    buf = torch.empty(means.shape[0], 1)
    assert ops.mip_filter_3d(means, table, out=buf) is buf and np.array_equal(buf.numpy(), ref["filter"])
    cams = cameras_of(table)
    assert torch.equal(ops.mip_camera_table(cams), table) and torch.equal(ops.mip_camera_table(iter(cams), "cpu"), table)
    param = mip.compute_3d_filter(iter(cams), types.SimpleNamespace(get_xyz=means))
    assert isinstance(param, torch.nn.Parameter) and not param.requires_grad and np.array_equal(param.numpy(), ref["filter"])
    batched = types.SimpleNamespace(R=table[:, :9].reshape(-1, 3, 3), T=table[:, 9:12], fx=table[:, 12], fy=table[:, 13],
                                    width=table[:, 14].to(torch.int32), height=table[:, 15].to(torch.int32))
    assert torch.equal(ops.mip_camera_table(batched), table)


def test_camera_table_reads_world_to_camera_of_a_fake_camera():
    from fakes import FakeCamera
    from gspl_amd import ops
    from oracle import gsplat_oracle as O
    cam = O.synthetic_camera(64, 48, 60.0, 59.0)
    row = ops.mip_camera_table([FakeCamera(cam, "cpu")])
    assert tuple(row.shape) == (1, 16) and row.dtype == torch.float32
    assert row[0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 4, 60, 59, 64, 48]


def test_no_row_valid_anywhere_keeps_the_initial_distance(ref):
    """The reference raises there (`max()` of an empty tensor); the op documents 100000 for every row."""
    from gspl_amd import ops
    means = torch.from_numpy(ref["means"][N_SEEN:])
    table = torch.from_numpy(ref["table"])
    filt, distance, valid = ops.mip_filter_3d(means, table, return_parts=True)
    assert not valid.any() and (distance == 100000.0).all()
    assert torch.equal(filt[:, 0], torch.full((means.shape[0],), 100000.0) / table[:, 12].max() * (0.2 ** 0.5))


@pytest.mark.parametrize("key,compensation,with_opacities", APPLY_CASES)
def test_cpu_apply_is_the_reference_bit_for_bit(ref, key, compensation, with_opacities):
    from gspl_amd import mip, ops
    t = lambda k: torch.from_numpy(ref[k])
    s, o = t("a_scales").requires_grad_(True), t("a_opacities").requires_grad_(True)
    new_s, second = ops.mip_apply_3d_filter(s, t("a_filter"), o if with_opacities else None, opacity_compensation=compensation)
    ((new_s * t("a_vs")).sum() + (second.reshape(-1) * t("a_vo")).sum()).backward()
    assert np.array_equal(new_s.detach().numpy(), ref[key + "_scales"]) and np.array_equal(s.grad.numpy(), ref[key + "_g_scales"])
    if with_opacities:
        assert np.array_equal(second.detach().numpy(), ref[key + "_opacities"]) and np.array_equal(o.grad.numpy(), ref[key + "_g_opacities"])
        theirs_o, theirs_s = mip.apply_3d_filter(filter_3d=t("a_filter"), opacities=t("a_opacities"), scales=t("a_scales"), opacity_compensation=compensation)
        assert torch.equal(theirs_o, second.detach()) and torch.equal(theirs_s, new_s.detach())
    else:
        assert np.array_equal(second.detach().numpy(), ref[key + "_coef"])
        assert torch.equal(mip.HipMipSplattingUtils.apply_3d_filter_on_scales(t("a_filter"), t("a_scales"), True)[1], second.detach())
        assert mip.apply_3d_filter_on_scales(t("a_filter"), t("a_scales"), False)[1] is None


def test_cpu_raw_inputs_are_the_activations_in_front(ref):
    from gspl_amd import ops
    g = torch.Generator().manual_seed(3)
    raw_s, raw_o, f = torch.randn(300, 3, generator=g) - 4, torch.randn(300, 1, generator=g), 0.05 * torch.rand(300, 1, generator=g)
    a = ops.mip_apply_3d_filter(raw_s, f, raw_o, raw_scales=True, raw_opacities=True)
    b = ops.mip_apply_3d_filter(torch.exp(raw_s), f, torch.sigmoid(raw_o))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and tuple(a[1].shape) == (300, 1)
    c = ops.mip_apply_3d_filter(raw_s, f[:, 0], raw_o[:, 0], raw_scales=True, opacity_compensation=False)
    assert torch.equal(c[0], b[0]) and c[1].shape == (300,) and torch.equal(c[1], raw_o[:, 0])


# ---- the reference's own classes next to the plugin's ---------------------------------------------------------------------------------
@needs_reference
def test_reference_methods_and_mixins_equal_the_plugins_bit_for_bit(worker):
    """`MipSplattingModel.get_3d_filtered_scales_and_opacities`, `MipSplattingRendererMixin.get_scales` / `get_opacities` and the
    appearance-Mip module's `get_scales`, unedited, against `gspl_amd`'s on the reference's model and on `HipMipSplattingModel`: values
    and the gradients of the stored scales and opacities.  The raw flags are taken for the reference's own activations and dropped for
    a pre-activated model."""
    assert len(worker["checks"]) == 4
    for key, got in worker["checks"].items():
        assert got["n_outputs"]["model"] == 4 and got["n_outputs"]["mixin"] == 4, key
        assert got["n_outputs"]["appearance"] == (3 if "compensation=True" in key else 2), key
        assert all(got["reference model"].values()) and all(got["hip model"].values()) and len(got["hip model"]) == 4, (key, got)
        assert worker["raw_flags"][key] == ([False, False] if "pre_activated=True" in key else [True, True]), key
    assert worker["get_opacities"] == [True, True]


@needs_reference
def test_configs_carry_the_reference_fields(worker):
    theirs, ours = worker["fields"]["model"]
    assert theirs == ours and list(theirs)[-2:] == ["filter_3d_update_interval", "opacity_compensation"]
    theirs, ours = worker["fields"]["v2"]
    # (separate_sh: this package's gsplat-v1 plugin reads shs_dc / shs_rest in place by default, the reference concatenates them)
    assert list(theirs) == list(ours) and all(ours[k] == theirs[k] for k in theirs if k != "separate_sh") and ours["filter_2d_kernel_size"] == 0.1
    theirs, ours = worker["fields"]["appearance_mip"]
    assert ours.pop("fused_mlp") is True and theirs == ours and ours["filter_2d_kernel_size"] == 0.1


@needs_reference
def test_training_setup_builds_the_table_once_and_the_filter_by_one_call(worker):
    t = worker["training_setup"]
    assert t["returned"] == ["optimizers", "schedulers"] and t["vanilla_called"] and t["tables_built"] == 1 and t["table_equal"]
    assert t["filter_is_golden"] and t["filter_is_reference"] and t["is_parameter"] and t["names"][-1] == "filter_3d"


@needs_reference
def test_checkpoints_load_strictly_both_ways(worker):
    assert worker["state_dict"] == {"keys_equal": True, "has_filter": True, "loaded": True, "values_equal": True}


def test_configs_instantiate():
    from gspl_amd import mip, renderers
    v1 = {f.name: f.default for f in dataclasses.fields(renderers.HipGSplatV1Renderer)}
    ours = {f.name: f.default for f in dataclasses.fields(renderers.HipGSplatMipSplattingRendererV2)}
    assert list(ours) == list(v1) and ours == {**v1, "filter_2d_kernel_size": 0.1}
    module = renderers.HipGSplatMipSplattingRendererV2(anti_aliased=False).instantiate()
    assert isinstance(module, renderers.HipGSplatMipSplattingRendererV2Module) and isinstance(module, renderers.HipGSplatV1RendererModule)
    assert type(module).__mro__[1] is renderers.HipMipSplattingRendererMixin and type(module).get_rgbs is renderers.HipGSplatV1RendererModule.get_rgbs
    cfg = renderers.HipGSplatAppearanceEmbeddingMipRenderer()
    assert cfg.filter_2d_kernel_size == 0.1 and isinstance(cfg.instantiate(), renderers.HipGSplatAppearanceEmbeddingRendererModule)
    with pytest.raises(ValueError, match="separate_sh"):
        renderers.HipGSplatAppearanceEmbeddingMipRenderer(separate_sh=False).instantiate()
    names = [f.name for f in dataclasses.fields(mip.HipMipSplatting)]
    assert names[-2:] == ["filter_3d_update_interval", "opacity_compensation"]
    assert (mip.HipMipSplatting().filter_3d_update_interval, mip.HipMipSplatting().opacity_compensation) == (100, True)


def test_stand_alone_instantiate_names_the_missing_module():
    from gspl_amd import mip
    if mip.INSIDE_REFERENCE:
        pytest.skip("the reference's internal package is importable in this process")
    with pytest.raises(RuntimeError, match=r"internal\.models\.mip_splatting"):
        mip.HipMipSplatting().instantiate()
    assert mip.HipMipSplattingModel is None


def test_a_model_without_a_filter_is_refused():
    from gspl_amd import renderers
    from fakes import FakeGaussianModel
    model = FakeGaussianModel(torch.zeros(4, 3), torch.ones(4, 3), torch.ones(4, 4), torch.ones(4, 1), torch.zeros(4, 16, 3))
    with pytest.raises(TypeError, match="3D filter"):
        renderers.HipGSplatMipSplattingRendererV2().instantiate().get_scales(None, model)
    with pytest.raises(TypeError, match="3D filter"):
        renderers.HipGSplatAppearanceEmbeddingMipRendererModule.get_scales(None, None, model)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_filter_refusals():
    from gspl_amd import ops
    means, table = torch.zeros(5, 3), torch.zeros(2, 16)
    with pytest.raises(TypeError, match="means must be a tensor"):
        ops.mip_filter_3d([[0., 0., 0.]], table)
    with pytest.raises(TypeError, match="camera_table must be a tensor"):
        ops.mip_filter_3d(means, None)
    with pytest.raises(ValueError, match=r"means must be \[N, 3\]"):
        ops.mip_filter_3d(torch.zeros(5, 4), table)
    with pytest.raises(ValueError, match=r"camera_table must be \[C, 16\]"):
        ops.mip_filter_3d(means, torch.zeros(2, 12))
    with pytest.raises(ValueError, match=r"camera_table must be \[C, 16\]"):
        ops.mip_filter_3d(means, torch.zeros(32))
    with pytest.raises(ValueError, match="at least one camera"):
        ops.mip_filter_3d(means, torch.zeros(0, 16))
    with pytest.raises(ValueError, match="1 .. 2\\^31 - 1 rows, got 0"):
        ops.mip_filter_3d(torch.zeros(0, 3), table)
    with pytest.raises(NotImplementedError, match="means must be float32"):
        ops.mip_filter_3d(means.double(), table)
    with pytest.raises(NotImplementedError, match="camera_table must be float32"):
        ops.mip_filter_3d(means, table.half())
    with pytest.raises(RuntimeError, match="camera_table is on meta, means on cpu"):
        ops.mip_filter_3d(means, table.to("meta"))
    for bad in (torch.empty(5), torch.empty(4, 1), torch.empty(5, 1, dtype=torch.float64)):
        with pytest.raises(ValueError, match="out must be"):
            ops.mip_filter_3d(means, torch.eye(16)[:2].contiguous(), out=bad)
    with pytest.raises(ValueError, match="at least one camera"):
        ops.mip_camera_table([])
    with pytest.raises(ValueError, match="camera 0 gives"):
        ops.mip_camera_table([types.SimpleNamespace(R=torch.eye(3), T=torch.zeros(2), fx=1., fy=1., width=4, height=4)])


def test_apply_refusals():
    from gspl_amd import ops
    s, f, o = torch.ones(5, 3), torch.ones(5, 1), torch.ones(5, 1)
    with pytest.raises(TypeError, match="scales must be a tensor"):
        ops.mip_apply_3d_filter(None, f, o)
    with pytest.raises(TypeError, match="raw_opacities without opacities"):
        ops.mip_apply_3d_filter(s, f, None, raw_opacities=True)
    with pytest.raises(ValueError, match=r"scales must be \[N, 3\]"):
        ops.mip_apply_3d_filter(torch.ones(5, 2), f, o)
    with pytest.raises(ValueError, match=r"filter_3d must be \[5, 1\] or \[5\]"):
        ops.mip_apply_3d_filter(s, torch.ones(4, 1), o)
    with pytest.raises(ValueError, match=r"opacities must be \[5, 1\] or \[5\]"):
        ops.mip_apply_3d_filter(s, f, torch.ones(5, 3))
    with pytest.raises(NotImplementedError, match="scales must be float32"):
        ops.mip_apply_3d_filter(s.double(), f, o)
    with pytest.raises(NotImplementedError, match="opacities must be float32"):
        ops.mip_apply_3d_filter(s, f, o.half())
    with pytest.raises(RuntimeError, match="filter_3d is on meta, scales on cpu"):
        ops.mip_apply_3d_filter(s, f.to("meta"), o)
    for launch in (ops.mip_apply_3d_filter_forward, lambda *a: ops.mip_apply_3d_filter_backward(*a, None, None)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            launch(s, f, o)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """The C entry points themselves (include/gspl_hip.h section 28): N or C out of range, a NULL required pointer, unknown flags and
    outputs that do not go with the inputs return the library's invalid-argument code; N = 0 succeeds in the apply calls.  None of
    these calls reaches the device."""
    import ctypes
    from gspl_amd import _lib as L
    for name in ("gspl_mip_filter3d", "gspl_mip_apply_fwd", "gspl_mip_apply_bwd"):
        assert name in L.exported_symbols()
    assert (L.GSPL_MIP_CAMERA_FLOATS, L.GSPL_MIP_WORKSPACE_BYTES, L.ABI_VERSION) == (16, 8, 39)
    lib = L.lib()
    block = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(block))
    bad = L.GSPL_ERR_INVALID_ARG
    filt = lambda N=4, C=2, means=p, cams=p, out=p, ws=p: lib.gspl_mip_filter3d(N, C, means, cams, out, None, None, ws, None)
    assert filt(N=0) == bad and filt(C=0) == bad and filt(N=2 ** 31) == bad and filt(N=-1) == bad
    assert filt(means=None) == bad and filt(cams=None) == bad and filt(out=None) == bad and filt(ws=None) == bad
    assert b"mip_filter3d" in lib.gspl_last_error()
    fwd = lambda N=4, flags=4, s=p, o=p, f=p, so=p, oo=p: lib.gspl_mip_apply_fwd(N, flags, s, o, f, so, oo, None)
    bwd = lambda N=4, flags=4, s=p, o=p, f=p, vs=p, vo=p: lib.gspl_mip_apply_bwd(N, flags, s, o, f, p, p, vs, vo, None)
    for call in (fwd, bwd):
        assert call(N=-1) == bad and call(flags=8) == bad and call(flags=2, o=None) == bad and call(s=None) == bad and call(f=None) == bad
        assert call(N=0) == L.GSPL_OK and call(N=0, flags=7) == L.GSPL_OK
    assert fwd(so=None) == bad and fwd(oo=None) == bad and fwd(flags=0, o=None) == bad
    assert bwd(vs=None) == bad and bwd(o=None) == bad and b"mip_apply_bwd" in lib.gspl_last_error()

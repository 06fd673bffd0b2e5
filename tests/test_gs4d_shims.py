"""No-GPU checks of the 4D-GS route: the HexPlane oracle against the reference's own double-precision run (tests/golden/ref_hexplane.npz,
written by tests/golden/make_hexplane_golden.py), the oracle's own sanity, the layout, the module's names against the reference's state
dict, the `cfg_args` reader, the refusals, the header and the launch hook."""
import json
import os
import subprocess
import sys
import textwrap
from argparse import Namespace

import numpy as np
import pytest
import torch

import hexplane_oracle as HO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")


def _default_args(**overrides):
    """`ModelHiddenParams` of 4DGaussians, the fields the deformation network reads."""
    args = dict(net_width=64, timebase_pe=4, defor_depth=1, posebase_pe=10, scale_rotation_pe=2, opacity_pe=2, timenet_width=64,
                timenet_output=32, bounds=1.6, grid_pe=0,
                kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 32, "resolution": [64, 64, 64, 25]},
                multires=[1, 2, 4, 8], no_dx=False, no_grid=False, no_ds=False, no_dr=False, no_do=True, no_dshs=True,
                empty_voxel=False, static_mlp=False, apply_rotation=False)
    args.update(overrides)
    return Namespace(**args)


GOLDEN_ARGS = dict(net_width=16, bounds=2.0, multires=[1, 2], no_do=False, no_dshs=False,
                   kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 8, "resolution": [5, 6, 7, 3]})


@pytest.fixture(scope="module")
def golden():
    d = dict(np.load(os.path.join(GOLDEN, "ref_hexplane.npz")))
    lay = HO.layout([5, 6, 7, 3], [1, 2], 8)
    grids = [[d[f"state/deformation_net.grid.grids.{level}.{p}"] for p in range(6)] for level in range(2)]
    return d, lay, grids, HO.pack(grids, lay)


def test_oracle_matches_the_reference_field(golden):
    d, lay, grids, table = golden
    assert d["x"].shape == (64, 3) and int((np.abs(d["x"]) > 2.0).any(axis=1).sum()) == 32 and np.abs(d["t"]).max() > 1.0
    aabb = d["state/deformation_net.grid.aabb"]
    assert aabb.tolist() == [[2.0] * 3, [-2.0] * 3]          # the MAXIMUM corner first: the sign flip
    r = HO.encode(d["x"], d["t"], table, aabb, lay, double=True)
    assert r.out.shape == d["field"].shape == (64, 16)
    assert np.abs(r.out - d["field"]).max() <= 1e-12
    # float32 coordinates (what the kernels are compared with) stay within float32 rounding of the same numbers
    r32 = HO.encode(d["x"], d["t"], table, aabb, lay)
    assert 0 < np.abs(r32.out - d["field"]).max() <= 1e-4


def test_network_forward_matches_the_reference_with_the_oracle_as_the_field(golden):
    """The module in double on CPU tensors up to the field call, which the oracle serves: every output within 1e-12 of the largest
    magnitude of the reference's tensor."""
    import gspl_amd  # noqa: F401
    from gspl_amd.gs4d import HipDeformNetwork
    d, lay, grids, table = golden
    net = HipDeformNetwork(_default_args(**GOLDEN_ARGS)).double()
    net.load_state_dict({k[len("state/"):]: torch.from_numpy(v) for k, v in d.items() if k.startswith("state/")}, strict=True)
    field = net.deformation_net.grid
    calls = []

    def oracle_field(pts, timestamps=None):
        calls.append(tuple(pts.shape))
        return torch.from_numpy(HO.encode(pts.numpy(), timestamps.numpy(), table, field.aabb.numpy(), lay, double=True).out)
    field.forward = oracle_field
    with torch.no_grad():
        outs = net(*(torch.from_numpy(d[k]) for k in ("x", "in_scales", "in_rotations", "in_opacity", "in_shs", "t")))
    assert calls == [(64, 3)]
    for name, got in zip(("means", "scales", "rotations", "opacity", "shs"), outs):
        ref = d["out_" + name]
        assert got.shape == ref.shape and np.abs(got.numpy() - ref).max() <= 1e-12 * np.abs(ref).max(), name


def test_oracle_constant_planes_and_finite_differences():
    lay = HO.layout([5, 6, 7, 3], [1, 2], 8)
    rng = np.random.default_rng(2)
    aabb = np.array([[2.0] * 3, [-2.0] * 3])
    x = (rng.random((50, 3)) * 6 - 3).astype(np.float32)
    t = (rng.random(50) * 3 - 1.5).astype(np.float32)
    r = HO.encode(x, t, np.full((lay.total, 8), 0.75), aabb, lay)
    assert np.abs(r.out - 0.75 ** 6).max() < 1e-14 and np.abs(r.out_abs - 0.75 ** 6).max() < 1e-14
    # odd multiples of 2^-10 strictly inside the box: with bounds 2 and R - 1 <= 13 every float32 step is exact, no pixel coordinate is
    # an integer, and a step of 2^-13 stays inside the cell
    x = ((2 * rng.integers(-1000, 1000, size=(50, 3)) + 1) / 1024.0).astype(np.float32)
    assert np.abs(x).max() < 2.0
    table, v = rng.standard_normal((lay.total, 8)), rng.standard_normal((50, 16))
    r = HO.encode(x, t, table, aabb, lay, v, want_x=True)
    assert int(r.v_table_count.sum()) <= 50 * 2 * 6 * 4 * 8 and r.v_table_count.sum() > 50 * 2 * 6 * 2 * 8
    step = np.float32(2.0 ** -13)
    for d in range(3):
        bump = np.zeros(3, dtype=np.float32)
        bump[d] = step
        fd = ((HO.encode(x + bump, t, table, aabb, lay).out - HO.encode(x - bump, t, table, aabb, lay).out) * v).sum(axis=1) / (2.0 * float(step))
        assert np.abs(fd - r.v_x[:, d]).max() <= 1e-6 * r.v_x_abs[:, d].max()          # the product of three planes is cubic along an axis
    # outside the box along x: the border texel, and no gradient along that axis
    far = np.array([[5.0, 0.1, 0.2], [-5.0, 0.1, 0.2]], dtype=np.float32)
    rf = HO.encode(far, 0.0, table, aabb, lay, np.ones((2, 16)), want_x=True)
    assert not rf.v_x[:, 0].any() and rf.v_x[:, 1:].all()
    # x = aabb[0] (the maximum corner) is -1: texel 0; x = aabb[1] is the LAST texel, whose second corner is no texel
    i0, f, inside = HO.pixels(HO.coordinates(np.array([[2.0, -2.0, 0.0]], dtype=np.float32), 0.0, aabb)[0][0, :3], 5)
    assert i0.tolist() == [0, 4, 2] and f.tolist() == [0.0, 0.0, 0.0] and inside.tolist() == [False, False, True]


def test_layout_matches_the_reference_shapes(golden):
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    d, olay, grids, table = golden
    lay = ops.hexplane_layout([5, 6, 7, 3], [1, 2], 8)
    assert lay.n_levels == 2 and lay.n_features == 8 and lay.n_output_dims == 16 and lay.total == olay.total == 161 + 536
    assert lay.resolutions.tolist() == [[5, 6, 7, 3], [10, 12, 14, 3]] and lay.resolutions.dtype == np.uint32 and lay.offsets.dtype == np.uint32
    assert [p[:2] for p in lay.planes[0]] == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    for level in range(2):
        assert [tuple(p) for p in lay.planes[level]] == [tuple(p) for p in olay.planes[level]]
        for p in range(6):
            a, b, Ra, Rb, first = lay.planes[level][p]
            assert grids[level][p].shape == lay.plane_shape(level, p) == (1, 8, Rb, Ra)          # [R_b, R_a]: axis a along the width
            assert lay.offsets[6 * level + p] == first and lay.offsets[6 * level + p + 1] == first + Ra * Rb
    assert lay.offsets[-1] == lay.total
    packed = ops.hexplane_pack([[torch.from_numpy(g) for g in level] for level in grids], lay)
    assert packed.shape == (lay.total, 8) and np.array_equal(packed.numpy(), table)
    leaves = [[torch.from_numpy(g).requires_grad_(True) for g in level] for level in grids]
    ops.hexplane_pack(leaves, lay).sum().backward()
    assert all(bool((g.grad == 1).all()) for level in leaves for g in level)
    big = ops.hexplane_layout([64, 64, 64, 150], [1, 2, 4, 8], 32)
    assert big.resolutions[3].tolist() == [512, 512, 512, 150] and big.total == sum(3 * (64 * m) ** 2 + 3 * 64 * m * 150 for m in (1, 2, 4, 8))


def test_state_dict_names_and_shapes_are_the_references():
    import gspl_amd  # noqa: F401
    from gspl_amd.gs4d import HipDeformNetwork
    want = json.load(open(os.path.join(GOLDEN, "gs4d_state_keys.json")))
    got = {k: list(v.shape) for k, v in HipDeformNetwork(_default_args()).state_dict().items()}
    assert got == want and list(got) == list(want)
    assert "deformation_net.grid.grids.3.5" in got and got["deformation_net.grid.grids.0.2"] == [1, 32, 25, 64]
    # the switches add the reference's names
    more = HipDeformNetwork(_default_args(static_mlp=True, empty_voxel=True, net_width=8, multires=[1],
                                          kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 8,
                                                          "resolution": [4, 4, 4, 2]})).state_dict()
    assert more["deformation_net.empty_voxel.grid"].shape == (1, 1, 64, 64, 64) and "deformation_net.static_mlp.3.weight" in more
    net = HipDeformNetwork(_default_args(net_width=8, multires=[1], kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4,
                                                                                    "output_coordinate_dim": 8, "resolution": [4, 4, 4, 2]}))
    planes = [p.detach() for p in net.deformation_net.grid.grids[0]]
    assert bool((planes[2] == 1).all()) and bool((planes[4] == 1).all()) and bool((planes[5] == 1).all())          # the time planes
    assert 0.1 <= float(planes[0].min()) and float(planes[0].max()) <= 0.5


CFG_ARGS = ("Namespace(sh_degree=3, source_path='/data/dnerf/lego', model_path='./output/dnerf/lego', images='images', resolution=-1, "
            "white_background=True, data_device='cuda', eval=True, render_process=False, add_points=False, extension='.png', llffhold=8, "
            "net_width=64, timebase_pe=4, defor_depth=0, posebase_pe=10, scale_rotation_pe=2, opacity_pe=2, timenet_width=64, "
            "timenet_output=32, bounds=1.6, plane_tv_weight=0.0001, time_smoothness_weight=0.01, l1_time_planes=0.0001, "
            "kplanes_config={'grid_dimensions': 2, 'input_coordinate_dim': 4, 'output_coordinate_dim': 32, 'resolution': [64, 64, 64, 25]}, "
            "multires=[1, 2], no_dx=False, no_grid=False, no_ds=False, no_dr=False, no_do=True, no_dshs=True, empty_voxel=False, grid_pe=0, "
            "static_mlp=False, apply_rotation=False, configs=None, expname='dnerf/lego', lambda_dssim=0, position_lr_init=0.00016)\n")


def test_cfg_args_are_parsed_and_never_evaluated(tmp_path):
    import gspl_amd  # noqa: F401
    from gspl_amd.gs4d import parse_cfg_args
    good = tmp_path / "cfg_args"
    good.write_text(CFG_ARGS)
    args = parse_cfg_args(str(good))
    assert isinstance(args, Namespace) and args.multires == [1, 2] and args.kplanes_config["resolution"] == [64, 64, 64, 25]
    assert args.no_do is True and args.configs is None and args.resolution == -1 and args.bounds == 1.6 and args.defor_depth == 0
    marker = tmp_path / "evaluated"
    for n, text in enumerate((
            f"Namespace(net_width=open({str(marker)!r}, 'w').write('x'))",
            f"Namespace(net_width=64, multires=[1, __import__('os').system('touch {marker}')])",
            f"open({str(marker)!r}, 'w').write('x')",
            f"Namespace(*[open({str(marker)!r}, 'w')])",
            "Namespace(net_width=width)",
            "import os")):
        bad = tmp_path / f"bad{n}"
        bad.write_text(text)
        with pytest.raises(ValueError):
            parse_cfg_args(str(bad))
    assert not marker.exists()


def test_cpu_tensors_and_unbuilt_options_are_refused():
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    from gspl_amd.gs4d import HipHexPlaneField
    lay = ops.hexplane_layout([5, 6, 7, 3], [1, 2], 8)
    table = torch.zeros(lay.total, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.hexplane_encode(torch.zeros(4, 3), 0.5, table, torch.tensor([[2.0] * 3, [-2.0] * 3]), lay)
    with pytest.raises(TypeError, match="layout"):
        ops.hexplane_encode(torch.zeros(4, 3), 0.5, table, torch.tensor([[2.0] * 3, [-2.0] * 3]), None)
    for F in (1, 4, 12, 128):
        with pytest.raises(NotImplementedError, match="output_coordinate_dim"):
            ops.hexplane_layout([5, 6, 7, 3], [1, 2], F)
    with pytest.raises(NotImplementedError, match="multires"):
        ops.hexplane_layout([5, 6, 7, 3], list(range(1, 10)), 8)
    with pytest.raises(NotImplementedError, match="input_coordinate_dim"):
        ops.hexplane_layout([5, 6, 7], [1], 8)
    with pytest.raises(NotImplementedError, match="grid_dimensions"):
        HipHexPlaneField(1.6, {"grid_dimensions": 3, "input_coordinate_dim": 4, "output_coordinate_dim": 8, "resolution": [4, 4, 4, 2]}, [1])
    with pytest.raises(ValueError, match="plane 2 of level 0"):
        ops.hexplane_pack([[torch.zeros(1, 8, 6, 5), torch.zeros(1, 8, 7, 5), torch.zeros(1, 8, 5, 3)] + [torch.zeros(1)] * 3] * 2, lay)
    box = ops.hexplane_box(torch.tensor([[2.0, 4.0, 8.0], [-2.0, -4.0, -8.0]]))
    assert box.dtype == np.float32 and box.tolist() == [2.0, 4.0, 8.0, -0.5, -0.25, -0.125]


def test_header_declares_the_entry_points():
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib as L
    text = open(L.HEADER_PATH).read()
    for name in ("gspl_hexplane_fwd", "gspl_hexplane_bwd"):
        assert f"int {name}(" in text and name in L.exported_symbols()
    section = text[text.index(" 22. The HexPlane"):]
    assert "PURELY ADDITIVE" in section and "no new struct" in section and L.ABI_VERSION == 39
    assert L._FUNCTIONS["gspl_hexplane_fwd"][2] == ("N", "F", "L", "resolutions", "offsets", "box", "x", "t", "t_uniform", "table", "out", "stream")
    assert L._FUNCTIONS["gspl_hexplane_bwd"][2][-5:] == ("table", "v_out", "v_table", "v_x", "stream")
    assert "hexplane.hip" in open(os.path.join(ROOT, "gaussian-splatting-lightning_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("switch", ["", "0", "1"])
def test_launch_hook_binds_the_plugin_only_when_asked(tmp_path, switch):
    """A fake `internal` package next to the script, as the reference's tree has it: with GSPL_HIP_GS4D=1 the launcher binds
    `internal.renderers.vanilla_gs4d_renderer.VanillaGS4DRenderer` to the plugin; unset or 0, the module is not even imported."""
    pkg = tmp_path / "internal" / "renderers"
    pkg.mkdir(parents=True)
    (tmp_path / "internal" / "__init__.py").write_text("")
    (pkg / "__init__.py").write_text("")
    (pkg / "vanilla_gs4d_renderer.py").write_text("class VanillaGS4DRenderer:\n    pass\n")
    script = tmp_path / "viewer.py"
    script.write_text(textwrap.dedent("""
        import sys, json
        early = "internal.renderers.vanilla_gs4d_renderer" in sys.modules
        from internal.renderers.vanilla_gs4d_renderer import VanillaGS4DRenderer
        print(json.dumps({"early": early, "cls": VanillaGS4DRenderer.__module__ + "." + VanillaGS4DRenderer.__name__}))
    """))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("GSPL_HIP_GS4D", None)
    if switch:
        env["GSPL_HIP_GS4D"] = switch
    r = subprocess.run([sys.executable, "-m", "gspl_amd.launch", str(script), "model", "--vanilla_gs4d"], capture_output=True, text=True,
                       env=env, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    if switch == "1":
        assert d == {"early": True, "cls": "gspl_amd.renderers.hip_vanilla_gs4d_renderer.HipVanillaGS4DRenderer"}
    else:
        assert d == {"early": False, "cls": "internal.renderers.vanilla_gs4d_renderer.VanillaGS4DRenderer"}

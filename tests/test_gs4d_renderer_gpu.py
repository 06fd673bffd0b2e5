"""HipVanillaGS4DRenderer on a synthetic 4DGaussians model directory (a `cfg_args` text, a seeded `deformation.pth` and the table file,
written into tmp_path): the five property tensors it hands to `HipVanillaRenderer.render` against the reference's formulation, restated
here with `F.grid_sample` in float32 torch on the GPU, and the image against the rasterizer called directly on those tensors.

Bound: |got - ref| <= 1e-5 rms(ref) per tensor — the forward bound of tests/test_hexplane.py (48 u on positive planes, 3e-6) carried
through float32 MLPs of width 32.  Where the torch formulation itself is not that close to its own float64 run, twice ITS float32-against-
float64 error instead: `empty_voxel` and `static_mlp` multiply the log-scales by a mask before the exponential, and on the MI355X the
torch formulation alone is 1.8e-5 rms (empty_voxel) and 8.3e-6 rms (static_mlp) from float64 on the activated scales; every other tensor
of every configuration is below 6e-6.  Measured there: the plugin's five tensors are BIT-EQUAL to the float32 torch formulation in all
five configurations (the kernel visits the corners in grid_sample's order with the same fma chain).  The test prints, per tensor, the
measured difference and the formulation's own error, both in units of rms(ref)."""
import itertools
import os
from argparse import Namespace

import pytest
import torch
import torch.nn.functional as F

from private_pool import private_memory_pool  # noqa: F401   (autouse: importing it is using it)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, W, H = 300, 64, 48

CONFIGS = {
    "as_shipped": dict(no_do=True, no_dshs=True),
    "everything_on": dict(no_do=False, no_dshs=False),
    "empty_voxel": dict(no_do=False, no_dshs=False, empty_voxel=True),
    "static_mlp": dict(no_do=False, no_dshs=False, static_mlp=True),
    "apply_rotation": dict(no_do=False, no_dshs=False, apply_rotation=True),
}


def _args(**overrides):
    args = dict(sh_degree=3, source_path="/data/scene", white_background=False, net_width=32, timebase_pe=4, defor_depth=2, posebase_pe=10,
                scale_rotation_pe=2, opacity_pe=2, timenet_width=16, timenet_output=8, bounds=1.6, grid_pe=0,
                kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 8, "resolution": [8, 9, 10, 4]},
                multires=[1, 2], no_dx=False, no_grid=False, no_ds=False, no_dr=False, no_do=True, no_dshs=True, empty_voxel=False,
                static_mlp=False, apply_rotation=False)
    args.update(overrides)
    return Namespace(**args)


def _model_dir(tmp_path, args, seed=5):
    """cfg_args as 4DGaussians writes it (the repr of the Namespace), a seeded state dict, the deformation table."""
    from gspl_amd.gs4d import HipDeformNetwork
    torch.manual_seed(seed)
    net = HipDeformNetwork(args)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for level in net.deformation_net.grid.grids:
            for plane in level:
                plane.copy_(0.6 + 0.8 * torch.rand(plane.shape, generator=g))          # the time planes too: the time must matter
        if args.empty_voxel:
            net.deformation_net.set_aabb([args.bounds] * 3, [-args.bounds] * 3)          # (registers xyz_min / xyz_max, as training does)
            net.deformation_net.empty_voxel.grid.copy_(0.5 + torch.rand(net.deformation_net.empty_voxel.grid.shape, generator=g))
    ckpt = tmp_path / "point_cloud" / "iteration_3000"
    ckpt.mkdir(parents=True)
    (tmp_path / "cfg_args").write_text(repr(args))
    torch.save(net.state_dict(), str(ckpt / "deformation.pth"))
    torch.save(torch.ones(N, dtype=torch.bool), str(ckpt / "deformation_table.pth"))
    return str(tmp_path)


class _Gaussians:
    """The surface of the reference's Gaussian model the renderer reads: RAW properties and the activations."""

    def __init__(self, seed=42):
        from gspl_amd import synthetic
        means, scales, quats, opac, shs = synthetic.scene(N, seed=seed)
        g = torch.Generator().manual_seed(seed)
        self.get_xyz = means.to(DEV)
        self.scales = torch.log(scales * 3).to(DEV)
        self.rotations = (quats * (0.5 + torch.rand(N, 1, generator=g))).to(DEV)          # not unit length: the activation has work to do
        self.opacities = torch.logit(opac.clamp(0.05, 0.95)).to(DEV)
        self.get_features = shs.to(DEV)
        self.active_sh_degree = 3
        self.scale_activation, self.opacity_activation, self.rotation_activation = torch.exp, torch.sigmoid, F.normalize


def _camera(time):
    from gspl_amd import synthetic
    cam = synthetic.CameraObject(synthetic.camera(W, H, 60.0), DEV)
    cam.time = torch.tensor(time, dtype=torch.float32, device=DEV)
    return cam


def _reference_formulation(state, args, pc, time, dtype):
    """The reference's call sequence (gs4d_hexplane.py, gs4d_deformation.py, vanilla_gs4d_renderer.py) on the state dict's tensors."""
    sd = {k: v.to(device=DEV, dtype=dtype) for k, v in state.items()}
    x, scales, rotations, opacity, shs = (t.to(dtype) for t in (pc.get_xyz, pc.scales, pc.rotations, pc.opacities, pc.get_features))
    aabb = sd["deformation_net.grid.aabb"]
    p4 = torch.cat([(x - aabb[0]) * (2.0 / (aabb[1] - aabb[0])) - 1.0, torch.full((N, 1), time, dtype=dtype, device=DEV)], dim=-1)
    levels = []
    for level in range(len(args.multires)):
        product = 1.0
        for p, (a, b) in enumerate(itertools.combinations(range(4), 2)):
            grid = sd[f"deformation_net.grid.grids.{level}.{p}"]
            sample = F.grid_sample(grid, p4[:, [a, b]].view(1, 1, N, 2), align_corners=True, mode="bilinear", padding_mode="border")
            product = product * sample.view(grid.shape[1], N).T
        levels.append(product)
    hidden = torch.cat(levels, dim=-1)

    def linear(prefix, i, h):
        return F.linear(h, sd[f"deformation_net.{prefix}.{i}.weight"], sd[f"deformation_net.{prefix}.{i}.bias"])

    def head(prefix, h):
        return linear(prefix, 3, F.relu(linear(prefix, 1, F.relu(h))))
    hidden = linear("feature_out", 0, hidden)
    for i in range(1, args.defor_depth):
        hidden = linear("feature_out", 2 * i, F.relu(hidden))
    if args.static_mlp:
        mask = head("static_mlp", hidden)
    elif args.empty_voxel:
        lo, hi = sd["deformation_net.empty_voxel.xyz_min"], sd["deformation_net.empty_voxel.xyz_max"]
        unit = ((x.reshape(1, 1, 1, N, 3) - lo) / (hi - lo)).flip((-1,)) * 2 - 1
        mask = F.grid_sample(sd["deformation_net.empty_voxel.grid"], unit, mode="bilinear", align_corners=True).reshape(1, N).T
    else:
        mask = torch.ones((N, 1), dtype=dtype, device=DEV)
    means = x * mask + head("pos_deform", hidden)
    new_scales = scales * mask + head("scales_deform", hidden)
    dr = head("rotations_deform", hidden)
    if args.apply_rotation:
        q1, q2 = rotations, dr
        new_rotations = torch.stack((q1[:, 0] * q2[:, 0] - q1[:, 1] * q2[:, 1] - q1[:, 2] * q2[:, 2] - q1[:, 3] * q2[:, 3],
                                     q1[:, 0] * q2[:, 1] + q1[:, 1] * q2[:, 0] + q1[:, 2] * q2[:, 3] - q1[:, 3] * q2[:, 2],
                                     q1[:, 0] * q2[:, 2] - q1[:, 1] * q2[:, 3] + q1[:, 2] * q2[:, 0] + q1[:, 3] * q2[:, 1],
                                     q1[:, 0] * q2[:, 3] + q1[:, 1] * q2[:, 2] - q1[:, 2] * q2[:, 1] + q1[:, 3] * q2[:, 0]), dim=1)
        new_rotations = new_rotations / torch.norm(new_rotations, dim=1, keepdim=True)
    else:
        new_rotations = rotations + dr
    new_shs = shs if args.no_dshs else shs * mask.unsqueeze(-1) + head("shs_deform", hidden).reshape(N, 16, 3)
    return {"means3D": means, "opacity": pc.opacity_activation(opacity),          # of the UNDEFORMED opacity, as the reference has it
            "scales": pc.scale_activation(new_scales), "rotations": pc.rotation_activation(new_rotations), "features": new_shs}


def _spy(monkeypatch):
    from gspl_amd.renderers import HipVanillaRenderer
    real, calls = HipVanillaRenderer.render, []

    def render(**kwargs):
        calls.append(kwargs)
        return real(**kwargs)
    monkeypatch.setattr(HipVanillaRenderer, "render", staticmethod(render))
    return real, calls


@pytest.mark.parametrize("name", list(CONFIGS))
def test_properties_match_the_reference_formulation_and_the_image_the_rasterizer(tmp_path, monkeypatch, name):
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipVanillaGS4DRenderer, Renderer
    args = _args(**CONFIGS[name])
    renderer = HipVanillaGS4DRenderer(_model_dir(tmp_path, args), 3000, DEV)
    assert isinstance(renderer, Renderer) and renderer.cfg_args == args and renderer.deformation_table.shape == (N,)
    state = torch.load(os.path.join(tmp_path, "point_cloud", "iteration_3000", "deformation.pth"), map_location="cpu")
    pc, cam, bg = _Gaussians(), _camera(0.3125), torch.tensor([0.1, 0.2, 0.3], device=DEV)
    real, calls = _spy(monkeypatch)
    with torch.no_grad():
        out = renderer(cam, pc, bg)
        ref32 = _reference_formulation(state, args, pc, 0.3125, torch.float32)
        ref64 = _reference_formulation(state, args, pc, 0.3125, torch.float64)
        direct = real(**calls[0])
    assert len(calls) == 1 and calls[0]["active_sh_degree"] == 3 and calls[0]["viewpoint_camera"] is cam
    for key, ref in ref32.items():
        got = calls[0][key]
        rms = float(ref64[key].pow(2).mean().sqrt())
        diff = float((got.double() - ref.double()).abs().max()) / rms
        own = float((ref.double() - ref64[key]).abs().max()) / rms
        print(f"{name} {key}: |plugin - torch f32| = {diff:.2e} rms, |torch f32 - torch f64| = {own:.2e} rms")
        assert got.shape == ref.shape and got.dtype == torch.float32 and diff <= max(1e-5, 2 * own), (key, diff, own)
    assert torch.equal(calls[0]["opacity"], torch.sigmoid(pc.opacities))
    assert out["render"].shape == (3, H, W) and torch.equal(out["render"], direct["render"]) and int((out["radii"] > 0).sum()) > 100
    assert float((out["render"] - bg.view(3, 1, 1)).abs().max()) > 0.05


def test_time_and_in_place_updates_reach_the_image(tmp_path, monkeypatch):
    """Another `camera.time` gives another image; an in-place edit of a plane parameter (what an optimizer step is) rebuilds the packed
    table; with nothing changed the table is the one kept."""
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipVanillaGS4DRenderer
    args = _args()
    renderer = HipVanillaGS4DRenderer(_model_dir(tmp_path, args), 3000, DEV)
    pc, bg = _Gaussians(), torch.zeros(3, device=DEV)
    real, calls = _spy(monkeypatch)
    field = renderer.deformation.deformation_net.grid
    with torch.no_grad():
        first = renderer(_camera(0.25), pc, bg)["render"].clone()
        table = field.packed()[0]
        again = renderer(_camera(0.25), pc, bg)["render"].clone()
        assert field.packed()[0] is table and torch.equal(first, again)
        later = renderer(_camera(0.875), pc, bg)["render"].clone()
        assert field.packed()[0] is table
        field.grids[1][3].mul_(1.25)
        edited = renderer(_camera(0.25), pc, bg)["render"].clone()
        assert field.packed()[0] is not table
    assert float((first - later).abs().max()) > 1e-3 and not torch.equal(calls[0]["means3D"], calls[2]["means3D"])
    assert float((first - edited).abs().max()) > 1e-3 and not torch.equal(calls[0]["means3D"], calls[3]["means3D"])

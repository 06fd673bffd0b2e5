"""The deformation network of 4D Gaussian Splatting (4DGaussians, arXiv 2310.08528) as the reference builds it
(internal/model_components/gs4d_deformation.py, gs4d_hexplane.py, gs4d_grid.py), with the HexPlane field on `ops.hexplane_encode` (HIP):

    HipDeformNetwork(args)          `deform_network`: (means, scales, rotations, opacity, shs, time) -> the five deformed tensors
      .deformation_net              HipDeformation: feature_out and the five small heads, plain `torch.nn` as in the reference
        .grid                       HipHexPlaneField: six planes per level, sampled and multiplied in ONE launch

The parameter and buffer names are the reference's (`deformation_net.grid.grids.{level}.{plane}`, `deformation_net.grid.aabb`,
`timenet.*`, `deformation_net.feature_out.*`, `deformation_net.{pos,scales,rotations,opacity,shs}_deform.*`, `*_poc`), so a
4DGaussians `deformation.pth` loads with `load_state_dict(strict=True)`.  `static_mlp`, the `empty_voxel` dense grid, `apply_rotation`,
`grid_pe` and every `no_*` switch are honoured, in torch, as the reference has them.

Two things the reference computes are left out because nothing reads them: the positional embeddings of the means, scales and
rotations (about 100 sin / cos values per Gaussian: `Deformation` uses only the first 3 / 4 columns, the raw values), and the
multiplication by a mask of ones when neither `static_mlp` nor `empty_voxel` is set (x * 1 is x, bit for bit).

The planes stay the module's parameters in the reference's channel-major shape [1, F, R_b, R_a]; the kernels read ONE channel-last
table packed from them.  It is kept while no plane has changed (tensor identity and version counter) and rebuilt after an in-place
update such as an optimizer step; with autograd on it is packed anew on every call, so that gradients reach the parameters."""
from __future__ import annotations

import ast
from argparse import Namespace

import torch
import torch.nn.functional as F
from torch import nn

from . import ops


def parse_cfg_args(path: str) -> Namespace:
    """The `cfg_args` of a 4DGaussians model directory: the text `Namespace(name=literal, ...)`.  Read with `ast`, literals only
    (numbers, strings, booleans, None, lists, tuples, dicts, sets): a file from a model directory is never evaluated.  Anything else
    — another call, a name, an attribute, an operator on names — raises ValueError."""
    with open(path, "r") as f:
        text = f.read()
    try:
        tree = ast.parse(text.strip(), mode="eval")
    except SyntaxError as e:
        raise ValueError(f"{path}: not a Namespace(...) expression: {e}") from e
    call = tree.body
    if not isinstance(call, ast.Call) or not isinstance(call.func, ast.Name) or call.func.id != "Namespace" or call.args:
        raise ValueError(f"{path}: expected Namespace(name=value, ...)")
    values = {}
    for keyword in call.keywords:
        if keyword.arg is None:
            raise ValueError(f"{path}: ** arguments are not read")
        try:
            values[keyword.arg] = ast.literal_eval(keyword.value)
        except (ValueError, TypeError, SyntaxError, MemoryError, RecursionError) as e:
            raise ValueError(f"{path}: the value of {keyword.arg!r} is not a literal") from e
    return Namespace(**values)


class HipHexPlaneField(nn.Module):
    """`HexPlaneField(bounds, planeconfig, multires)`: `grids[level][plane]` [1, F, R_b, R_a] for the planes xy, xz, xt, yz, yt, zt,
    the multiplier of a level on the spatial axes only, `aabb` [2, 3] with the MAXIMUM corner first (so the normalised coordinates
    carry the reference's sign flip), features of the levels concatenated."""

    def __init__(self, bounds, planeconfig, multires) -> None:
        super().__init__()
        self.aabb = nn.Parameter(torch.tensor([[bounds] * 3, [-bounds] * 3], dtype=torch.float32), requires_grad=False)
        self.grid_config = [planeconfig]
        self.multiscale_res_multipliers = list(multires)
        self.concat_features = True
        if planeconfig.get("grid_dimensions", 2) != 2:
            raise NotImplementedError(f"HipHexPlaneField: grid_dimensions 2 is built, got {planeconfig['grid_dimensions']}")
        if planeconfig.get("input_coordinate_dim", 4) != 4:
            raise NotImplementedError(f"HipHexPlaneField: input_coordinate_dim 4 is built, got {planeconfig['input_coordinate_dim']}")
        self.layout = ops.hexplane_layout(planeconfig["resolution"], self.multiscale_res_multipliers, planeconfig["output_coordinate_dim"])
        self.grids = nn.ModuleList()
        for level in range(self.layout.n_levels):
            planes = nn.ParameterList()
            for plane, (a, b) in enumerate(ops.hexplane.PLANES):
                coef = nn.Parameter(torch.empty(self.layout.plane_shape(level, plane)))
                if b == 3:          # the planes that hold the time start at one
                    nn.init.ones_(coef)
                else:
                    nn.init.uniform_(coef, a=0.1, b=0.5)
                planes.append(coef)
            self.grids.append(planes)
        self.feat_dim = self.layout.n_output_dims
        self._packed = None          # (key, table, box)

    @property
    def get_aabb(self):
        return self.aabb[0], self.aabb[1]

    def set_aabb(self, xyz_max, xyz_min):
        self.aabb = nn.Parameter(torch.tensor([xyz_max, xyz_min], dtype=torch.float32, device=self.aabb.device), requires_grad=False)

    def _planes(self):
        return [list(level) for level in self.grids]

    def packed(self):
        """(table [total, F], box [6] on the host).  Without autograd the pair is kept while every plane and the box are the tensors
        they were, at the version they had."""
        planes = self._planes()
        if torch.is_grad_enabled() and any(p.requires_grad for level in planes for p in level):
            return ops.hexplane_pack(planes, self.layout), ops.hexplane_box(self.aabb)
        key = tuple((id(p), p._version, p.data_ptr()) for level in planes for p in level) + ((id(self.aabb), self.aabb._version, self.aabb.data_ptr()),)
        if self._packed is None or self._packed[0] != key:
            with torch.no_grad():
                self._packed = (key, ops.hexplane_pack(planes, self.layout).contiguous(), ops.hexplane_box(self.aabb))
        return self._packed[1], self._packed[2]

    def forward(self, pts: torch.Tensor, timestamps=None) -> torch.Tensor:
        """pts [N, 3]; timestamps a python number (ONE time for the call), or a tensor [N, 1] / [N] with one per point -> [N, L F]."""
        if timestamps is None:
            raise ValueError("HipHexPlaneField: the field has time planes and needs timestamps")
        table, box = self.packed()
        pts = pts.reshape(-1, pts.shape[-1])
        if isinstance(timestamps, torch.Tensor) and timestamps.numel() == 1 and pts.shape[0] != 1:
            timestamps = float(timestamps)
        return ops.hexplane_encode(pts, timestamps, table, box, self.layout)

    def get_density(self, pts, timestamps=None):
        return self(pts, timestamps)


class DenseGrid(nn.Module):
    """The `empty_voxel` grid: one trilinear `F.grid_sample` (align_corners=True) of `grid` [1, C, *world_size] inside the box that
    `set_aabb` registers as the buffers `xyz_min` / `xyz_max`.  A state dict that carries the two buffers (one saved after `set_aabb`)
    registers them on loading; one without them loads too, as in the reference, and the grid cannot be sampled until `set_aabb`."""

    def __init__(self, channels, world_size, **kwargs):
        super().__init__()
        self.channels = channels
        self.world_size = world_size
        self.grid = nn.Parameter(torch.ones([1, channels, *world_size]))

    def set_aabb(self, xyz_max, xyz_min):
        self.register_buffer("xyz_min", torch.as_tensor(xyz_min, dtype=torch.float32).to(self.grid.device))
        self.register_buffer("xyz_max", torch.as_tensor(xyz_max, dtype=torch.float32).to(self.grid.device))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        if prefix + "xyz_min" in state_dict and prefix + "xyz_max" in state_dict and not hasattr(self, "xyz_min"):
            self.set_aabb(state_dict[prefix + "xyz_max"], state_dict[prefix + "xyz_min"])
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, xyz):
        lead = xyz.shape[:-1]
        unit = (xyz.reshape(1, 1, 1, -1, 3) - self.xyz_min) / (self.xyz_max - self.xyz_min)
        out = F.grid_sample(self.grid, unit.flip((-1,)) * 2 - 1, mode="bilinear", align_corners=True)
        return out.reshape(self.channels, -1).T.reshape(*lead, self.channels)

    def extra_repr(self):
        return f"channels={self.channels}, world_size={self.world_size}"


def _head(width: int, n_out: int) -> nn.Sequential:
    return nn.Sequential(nn.ReLU(), nn.Linear(width, width), nn.ReLU(), nn.Linear(width, n_out))


def frequency_embedding(values: torch.Tensor, frequencies) -> torch.Tensor:
    """`poc_fre`: [values | sin(values f) | cos(values f)] over the frequencies f, flattened per row."""
    scaled = (values.unsqueeze(-1) * frequencies).flatten(-2)
    return torch.cat([values, scaled.sin(), scaled.cos()], -1)


def quaternion_product_normalized(q1: torch.Tensor, q2: torch.Tensor) -> torch.Tensor:
    """The Hamilton product of two batches [N, 4] (w, x, y, z), normalised: the `apply_rotation` form of the rotation update."""
    w1, x1, y1, z1 = q1[:, 0], q1[:, 1], q1[:, 2], q1[:, 3]
    w2, x2, y2, z2 = q2[:, 0], q2[:, 1], q2[:, 2], q2[:, 3]
    q = torch.stack((w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2,
                     w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2), dim=1)
    return q / torch.norm(q, dim=1, keepdim=True)


class HipDeformation(nn.Module):
    """`Deformation(D, W, ..., grid_pe, args)`: the field, `feature_out` (D linear layers of width W) and one two-layer head per
    deformed property."""

    def __init__(self, D=8, W=256, input_ch=27, input_ch_time=9, grid_pe=0, skips=(), args=None):
        super().__init__()
        self.D, self.W, self.input_ch, self.input_ch_time, self.skips, self.grid_pe = D, W, input_ch, input_ch_time, list(skips), grid_pe
        self.args = args
        self.no_grid = args.no_grid
        self.grid = HipHexPlaneField(args.bounds, args.kplanes_config, args.multires)
        if args.empty_voxel:
            self.empty_voxel = DenseGrid(channels=1, world_size=[64, 64, 64])
        if args.static_mlp:
            self.static_mlp = _head(W, 1)
        self.ratio = 0
        n_in = 4 if self.no_grid else self.grid.feat_dim * (3 if grid_pe != 0 else 1)
        layers = [nn.Linear(n_in, W)]
        for _ in range(D - 1):
            layers += [nn.ReLU(), nn.Linear(W, W)]
        self.feature_out = nn.Sequential(*layers)
        self.pos_deform = _head(W, 3)
        self.scales_deform = _head(W, 3)
        self.rotations_deform = _head(W, 4)
        self.opacity_deform = _head(W, 1)
        self.shs_deform = _head(W, 16 * 3)

    @property
    def get_aabb(self):
        return self.grid.get_aabb

    @property
    def get_empty_ratio(self):
        return self.ratio

    def set_aabb(self, xyz_max, xyz_min):
        self.grid.set_aabb(xyz_max, xyz_min)
        if self.args.empty_voxel:
            self.empty_voxel.set_aabb(xyz_max, xyz_min)

    def query_time(self, means, time):
        """time: a python number for the whole call, or [N, 1]."""
        if self.no_grid:
            if not isinstance(time, torch.Tensor) or time.numel() == 1:
                time = torch.as_tensor(time, dtype=means.dtype, device=means.device).reshape(1, 1).expand(means.shape[0], 1)
            features = torch.cat([means[:, :3], time[:, :1]], -1)
        else:
            features = self.grid(means[:, :3], time if not isinstance(time, torch.Tensor) else time[:, :1])
            if self.grid_pe > 1:
                features = frequency_embedding(features, self.grid_pe)
        return self.feature_out(features)

    def forward(self, means, scales=None, rotations=None, opacity=None, shs=None, time_feature=None, time=None):
        if time is None:
            raise NotImplementedError("HipDeformation: the static form (no time) is not built; the reference's needs a 3-D field")
        return self.forward_dynamic(means, scales, rotations, opacity, shs, time_feature, time)

    def forward_dynamic(self, means, scales, rotations, opacity, shs, time_feature, time):
        args = self.args
        hidden = self.query_time(means, time)
        if args.static_mlp:
            mask = self.static_mlp(hidden)
        elif args.empty_voxel:
            mask = self.empty_voxel(means[:, :3])
        else:
            mask = None          # a mask of ones in the reference

        def masked(value, m):
            return value if m is None else value * m

        new_means = means[:, :3] if args.no_dx else masked(means[:, :3], mask) + self.pos_deform(hidden)
        new_scales = scales[:, :3] if args.no_ds else masked(scales[:, :3], mask) + self.scales_deform(hidden)
        if args.no_dr:
            new_rotations = rotations[:, :4]
        elif args.apply_rotation:
            new_rotations = quaternion_product_normalized(rotations, self.rotations_deform(hidden))
        else:
            new_rotations = rotations[:, :4] + self.rotations_deform(hidden)
        new_opacity = opacity[:, :1] if args.no_do else masked(opacity[:, :1], mask) + self.opacity_deform(hidden)
        if args.no_dshs:
            new_shs = shs
        else:
            new_shs = masked(shs, None if mask is None else mask.unsqueeze(-1)) + self.shs_deform(hidden).reshape([shs.shape[0], 16, 3])
        return new_means, new_scales, new_rotations, new_opacity, new_shs

    def get_mlp_parameters(self):
        return [p for name, p in self.named_parameters() if "grid" not in name]

    def get_grid_parameters(self):
        return [p for name, p in self.named_parameters() if "grid" in name]


def _xavier(module):
    if isinstance(module, nn.Linear):
        nn.init.xavier_uniform_(module.weight, gain=1)


class HipDeformNetwork(nn.Module):
    """`deform_network(args)`.  `timenet` and the `*_poc` buffers exist because the checkpoints carry them; nothing reads their output
    in the reference's forward either."""

    def __init__(self, args):
        super().__init__()
        self.timenet = nn.Sequential(nn.Linear(2 * args.timebase_pe + 1, args.timenet_width), nn.ReLU(),
                                     nn.Linear(args.timenet_width, args.timenet_output))
        self.deformation_net = HipDeformation(W=args.net_width, D=args.defor_depth, input_ch=3 + 3 * args.posebase_pe * 2, grid_pe=args.grid_pe,
                                              input_ch_time=args.timenet_output, args=args)
        for name, count in (("time_poc", args.timebase_pe), ("pos_poc", args.posebase_pe), ("rotation_scaling_poc", args.scale_rotation_pe),
                            ("opacity_poc", args.opacity_pe)):
            self.register_buffer(name, torch.tensor([float(2 ** i) for i in range(count)], dtype=torch.float32))
        self.apply(_xavier)

    @property
    def get_aabb(self):
        return self.deformation_net.get_aabb

    @property
    def get_empty_ratio(self):
        return self.deformation_net.get_empty_ratio

    def forward(self, point, scales=None, rotations=None, opacity=None, shs=None, times_sel=None):
        return self.forward_dynamic(point, scales, rotations, opacity, shs, times_sel)

    def forward_dynamic(self, point, scales=None, rotations=None, opacity=None, shs=None, times_sel=None):
        """times_sel: ONE python number for the call (what a renderer has: one time per frame), or a tensor [N, 1]."""
        return self.deformation_net(point, scales, rotations, opacity, shs, None, times_sel)

    def get_mlp_parameters(self):
        return self.deformation_net.get_mlp_parameters() + list(self.timenet.parameters())

    def get_grid_parameters(self):
        return self.deformation_net.get_grid_parameters()

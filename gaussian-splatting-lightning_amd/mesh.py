"""Mesh extraction from a trained 2DGS model: render the training views, fuse their depth maps into a truncated signed distance
volume, take its zero level set, colour it, drop the floaters, write `.ply` files.  The GPU work is two HIP kernels
(`ops.tsdf_fuse`, `ops.marching_tetrahedra`; include/gspl_hip.h section 18); nothing here needs open3d, trimesh or skimage.

    python -m gspl_amd.mesh MODEL_PATH [--dataset_path P] [--voxel_size S] [--depth_trunc D] [--sdf_trunc T] [--num_cluster 50]
                                       [--unbounded] [--mesh_res 1024]

writes `fuse.ply` (or `fuse_unbounded.ply`) and the `_post.ply` file next to the model, as the reference's
`internal/entrypoints/gs2d_mesh_extraction.py` does (same arguments and defaults).

What differs from the reference, on purpose:
  * the iso-surface is marching TETRAHEDRA (six per cell), not marching cubes: no case table, no ambiguous case, a closed
    2-manifold wherever the surface stays inside the volume — and about three times as many triangles for the same lattice;
  * views are fused stack by stack of equal image size, not strictly in camera order.  The running mean is the same number;
    its rounding depends on the order when a scene mixes image sizes;
  * the bounded mode runs the SAME kernels as the unbounded one, without contraction, on a dense lattice over the cameras' bounding
    sphere, with the `depth_trunc` cut.  The reference hands this mode to Open3D's `ScalableTSDFVolume` (8-bit colours, its own
    weighting and marching cubes): PARITY WITH OPEN3D IS UNPINNED — Open3D cannot be installed next to this package's tests;
  * like the reference's torch path, the volume starts at tsdf = 1 with weight 1.  Behind a surface, past the truncation band,
    no view counts and the value stays 1: a thin second shell appears there (outside -> inside -> "outside" again).
    `keep_largest_clusters` removes it when it is asked for fewer clusters; it is a property of the published algorithm."""
from __future__ import annotations

import argparse
import os
import sys
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import ops
from .formats import write_ply_mesh


@dataclass
class MapStack:
    """The maps of the cameras `indices` (all of one image size), on the device: rgb [V, 3, H, W], depth [V, H, W]."""
    indices: List[int]
    rgb: Tensor
    depth: Tensor


def stack_maps(rgbmaps: Sequence[Tensor], depthmaps: Sequence[Tensor], device=None) -> List[MapStack]:
    """Per-camera maps ([3, H, W] and [1, H, W] or [H, W]) stacked per image size, in order of first appearance."""
    groups: dict = {}
    for i, (rgb, depth) in enumerate(zip(rgbmaps, depthmaps)):
        depth = depth.reshape(depth.shape[-2:])
        groups.setdefault(tuple(depth.shape), []).append((i, rgb, depth))
    stacks = []
    for members in groups.values():
        rgb = torch.stack([m[1] for m in members]).float()
        depth = torch.stack([m[2] for m in members]).float()
        if device is not None:
            rgb, depth = rgb.to(device), depth.to(device)
        stacks.append(MapStack([m[0] for m in members], rgb.contiguous(), depth.contiguous()))
    return stacks


def _stacks(maps) -> List[MapStack]:
    if isinstance(maps, (list, tuple)) and len(maps) > 0 and all(isinstance(m, MapStack) for m in maps):
        return list(maps)
    rgbmaps, depthmaps = maps          # the reference's (rgbmaps, depthmaps)
    return stack_maps(rgbmaps, depthmaps, device="cuda")


@torch.no_grad()
def render_views(model, renderer, cameras: Iterable, bg_color: Tensor) -> List[MapStack]:
    """Colour and `surf_depth` of every camera, kept on the device and stacked per image size."""
    rgbmaps, depthmaps = [], []
    for camera in cameras:
        out = renderer(camera, model, bg_color)
        rgbmaps.append(out["render"].detach())
        depthmaps.append(out["surf_depth"].detach())
    return stack_maps(rgbmaps, depthmaps)


def focus_point_fn(poses: np.ndarray) -> np.ndarray:
    """The point nearest to all optical axes of `poses` [N, 3, 4] (least squares)."""
    directions, origins = poses[:, :3, 2:3], poses[:, :3, 3:4]
    m = np.eye(3) - directions * np.transpose(directions, [0, 2, 1])
    mt_m = np.transpose(m, [0, 2, 1]) @ m
    return np.linalg.inv(mt_m.mean(0)) @ (mt_m @ origins).mean(0)[:, 0]


@torch.no_grad()
def estimate_bounding_sphere(cameras: Iterable) -> Tuple[np.ndarray, float]:
    """(center [3] float64, radius): the focus point of the cameras and the distance of the nearest camera to it."""
    c2ws = np.array([np.linalg.inv(np.asarray(cam.world_to_camera.T.detach().cpu().double().numpy())) for cam in cameras])
    poses = c2ws[:, :3, :] @ np.diag([1.0, -1.0, -1.0, 1.0])
    center = focus_point_fn(poses)
    radius = float(np.linalg.norm(c2ws[:, :3, 3] - center, axis=-1).min())
    return center, radius


def contract(x: Tensor) -> Tensor:
    mag = torch.linalg.norm(x, dim=-1, keepdim=True)
    return torch.where(mag < 1, x, (2 - 1 / mag) * (x / mag))


def uncontract(y: Tensor) -> Tensor:
    mag = torch.linalg.norm(y, dim=-1, keepdim=True)
    return torch.where(mag < 1, y, (1 / (2 - mag)) * (y / mag))


def _views(cameras, indices, device) -> Tensor:
    return torch.stack([cameras[i].full_projection.detach().to(device=device, dtype=torch.float32) for i in indices]).contiguous()


def _fuse_stacks(state, table, stacks, cameras, with_rgb=False, **samples):
    for stack in stacks:
        ops.tsdf_fuse(state, table, _views(cameras, stack.indices, table.device), stack.depth, stack.rgb if with_rgb else None, **samples)
    return state


def _blocks(nodes: int, crop: int):
    """Blocks of at most `crop` nodes that share their boundary planes: (offset, size) per axis."""
    out, start = [], 0
    while True:
        size = min(crop, nodes - start)
        out.append((start, size))
        if start + size >= nodes:
            return out
        start += size - 1


def _level_set(table: Tensor, nodes: Tuple[int, int, int], crop: int, stacks, cameras, lo: Tensor, hi: Tensor, level: float = 0.0):
    """Fuse and mesh the lattice block by block; the soups of the blocks are merged through their edge keys."""
    dev = table.device
    step = (hi - lo) / torch.tensor([max(n - 1, 1) for n in nodes], dtype=torch.float32, device=dev)
    soups = []
    for b0, m0 in _blocks(nodes[0], crop):
        for b1, m1 in _blocks(nodes[1], crop):
            for b2, m2 in _blocks(nodes[2], crop):
                state = ops.tsdf_init(m0 * m1 * m2, False, dev)
                _fuse_stacks(state, table, stacks, cameras, lattice=nodes, block=((b0, b1, b2), (m0, m1, m2)))
                # a block the level does not cross (the reference's min / max test) counts zero triangles and emits nothing
                soups.append(ops.marching_tetrahedra_soup(state[0].view(m0, m1, m2), level, lo, step, nodes, (b0, b1, b2)))
                del state
    vertices, faces, _ = ops.index_soup(torch.cat([s[0] for s in soups]), torch.cat([s[1] for s in soups]))
    return vertices, faces


def _colours(vertices: Tensor, voxel_size, stacks, cameras) -> Tensor:
    """The reference's colouring: a second fusion at the world-space vertices, no contraction."""
    state = ops.tsdf_init(vertices.shape[0], True, vertices.device)
    table = ops.tsdf_table(voxel_size=voxel_size, with_rgb=True, device=vertices.device)
    _fuse_stacks(state, table, stacks, cameras, with_rgb=True, points=vertices.contiguous())
    return state[2]


def _quantile(x: Tensor, q: float) -> Tensor:
    """np.quantile's linear rule on the device (torch.quantile refuses more than 2^24 elements)."""
    s = torch.sort(x.reshape(-1)).values
    pos = q * (s.numel() - 1)
    i = int(pos)
    j = min(i + 1, s.numel() - 1)
    return s[i] + (s[j] - s[i]) * (pos - i)


@torch.no_grad()
def extract_mesh_unbounded(maps, bound, cameras, model, resolution: int = 1024, crop: int = 512, max_range: float = 32.0):
    """The reference's `extract_mesh_unbounded`: the level set of the TSDF on a lattice in CONTRACTED space.  Returns
    (vertices [Nv, 3] world space, faces [T, 3] int64, colors [Nv, 3]) on the device.

    The lattice spans [-R, R]^3, R the 0.95 quantile of the contracted Gaussian centres (+0.01, at most 1.9), in
    `resolution // crop` blocks of `crop` nodes per axis that share their boundary planes."""
    stacks = _stacks(maps)
    dev = stacks[0].depth.device
    center, radius = bound
    center = torch.as_tensor(np.asarray(center.detach().cpu()) if isinstance(center, Tensor) else center, dtype=torch.float32).to(dev)
    radius = float(radius)
    if resolution < 2 or crop < 2:
        raise ValueError("resolution and crop must be at least 2")
    voxel_size = radius * 2 / resolution
    means = model.get_xyz.detach().to(dev).float()
    R = _quantile(torch.linalg.norm(contract((means - center) / radius), dim=-1), 0.95)
    R = torch.clamp(R + 0.01, max=1.9)
    n = max(resolution // crop, 1) * (crop - 1) + 1
    lo, hi = -R.expand(3).contiguous(), R.expand(3).contiguous()
    table = ops.tsdf_table(center, radius, voxel_size, contract=True, lo=lo, hi=hi, device=dev)
    vertices, faces = _level_set(table, (n, n, n), crop, stacks, cameras, lo, hi)
    vertices = torch.clamp(uncontract(vertices) * radius + center, -max_range, max_range)
    return vertices, faces, _colours(vertices, voxel_size, stacks, cameras)


@torch.no_grad()
def extract_mesh_bounded(maps, cameras, voxel_size: float = 0.004, sdf_trunc: float = 0.02, depth_trunc: float = 3.0, center=(0.0, 0.0, 0.0),
                         radius: float = 1.0, crop: int = 512):
    """TSDF fusion with a fixed truncation on a dense lattice of spacing `voxel_size` over the box of the bounding sphere
    (`center`, `radius`: host numbers, as `estimate_bounding_sphere` returns them); depth beyond `depth_trunc` is ignored.  Returns
    (vertices, faces, colors) on the device.  Open3D's result for the same arguments is NOT pinned (module text)."""
    stacks = _stacks(maps)
    dev = stacks[0].depth.device
    center = np.asarray(center.detach().cpu() if isinstance(center, Tensor) else center, dtype=np.float64).reshape(3)
    radius, voxel_size = float(radius), float(voxel_size)
    if voxel_size <= 0 or radius <= 0:
        raise ValueError("voxel_size and radius must be positive")
    n = int(np.ceil(2 * radius / voxel_size - 1e-6)) + 1
    lo = torch.tensor(center - radius, dtype=torch.float32, device=dev)
    hi = torch.tensor(center - radius + (n - 1) * voxel_size, dtype=torch.float32, device=dev)
    table = ops.tsdf_table(voxel_size=voxel_size, sdf_trunc=sdf_trunc, depth_trunc=depth_trunc, lo=lo, hi=hi, device=dev)
    vertices, faces = _level_set(table, (n, n, n), crop, stacks, cameras, lo, hi)
    return vertices, faces, _colours(vertices, voxel_size, stacks, cameras)


def face_clusters(faces: Tensor, n_vertices: int) -> Tensor:
    """A label per face, equal for faces connected through shared edges: the smallest face index of the cluster.  Label
    propagation over the edge table with pointer jumping, torch only."""
    T = faces.shape[0]
    labels = torch.arange(T, dtype=torch.int64, device=faces.device)
    if T == 0:
        return labels
    pairs = torch.stack([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], dim=1)          # [T, 3, 2]
    edge_key = pairs.min(dim=-1).values * n_vertices + pairs.max(dim=-1).values                     # [T, 3]
    n_edges_of, edge = torch.unique(edge_key.reshape(-1), return_inverse=True)
    edge = edge.reshape(T, 3)
    n_edges = n_edges_of.shape[0]
    while True:
        low = torch.full((n_edges,), T, dtype=torch.int64, device=faces.device)
        low.scatter_reduce_(0, edge.reshape(-1), labels.repeat_interleave(3), reduce="amin")
        new = torch.minimum(labels, low[edge].min(dim=1).values)
        new = new[new]                      # pointer jumping: a label is a face index
        if torch.equal(new, labels):
            return labels
        labels = new


def keep_largest_clusters(vertices: Tensor, faces: Tensor, cluster_to_keep: int = 50, min_triangles: int = 50, colors: Optional[Tensor] = None):
    """The reference's `post_process_mesh`: keep the clusters (faces connected through shared edges) with at least
    max(size of the `cluster_to_keep`-th largest, `min_triangles`) triangles — `min_triangles` alone when there are fewer clusters
    than that (the reference raises there) — and drop the vertices nothing refers to.  Returns (vertices, faces), or
    (vertices, faces, colors) when colours are given."""
    labels = face_clusters(faces, vertices.shape[0])
    _, cluster, sizes = torch.unique(labels, return_inverse=True, return_counts=True)
    threshold = min_triangles
    if 1 <= cluster_to_keep <= sizes.numel():
        threshold = max(int(torch.sort(sizes, descending=True).values[cluster_to_keep - 1]), min_triangles)
    faces = faces[sizes[cluster] >= threshold]
    used = torch.zeros(vertices.shape[0], dtype=torch.bool, device=vertices.device)
    used[faces.reshape(-1)] = True
    remap = torch.cumsum(used, 0) - 1
    out = (vertices[used], remap[faces])
    return out if colors is None else out + (colors[used],)


def _load(model_path: str, dataset_path: Optional[str], device):
    """Model, renderer and training cameras through the reference's loader and data parser."""
    from . import compat
    compat.install()
    try:
        from internal.utils.gaussian_model_loader import GaussianModelLoader
    except ImportError as e:
        raise SystemExit("gspl_amd.mesh loads checkpoints and datasets through the reference project (internal.utils.gaussian_model_loader, "
                         f"internal.dataparsers), which is not importable here ({e}).  Put the reference tree on PYTHONPATH, or call "
                         "gspl_amd.mesh.render_views / extract_mesh_bounded / extract_mesh_unbounded with your own model and cameras.")
    load_file = GaussianModelLoader.search_load_file(model_path)
    parser_config = None
    if load_file.endswith(".ckpt"):
        ckpt = torch.load(load_file, map_location="cpu", weights_only=False)
        model = GaussianModelLoader.initialize_model_from_checkpoint(ckpt, device=device)
        model.freeze()
        model.pre_activate_all_properties()
        renderer = GaussianModelLoader.initialize_renderer_from_checkpoint(ckpt, stage="validate", device=device)
        parser_config = ckpt.get("datamodule_hyper_parameters", {}).get("parser")
        if dataset_path is None:
            dataset_path = ckpt["datamodule_hyper_parameters"]["path"]
    else:
        if dataset_path is None:
            raise SystemExit("a .ply model carries no dataset path: give --dataset_path")
        model, renderer = GaussianModelLoader.initialize_model_and_renderer_from_ply_file(load_file, device=device, eval_mode=True, pre_activate=True)
    if parser_config is None:
        from internal.dataparsers.colmap_dataparser import Colmap
        parser_config = Colmap()
    outputs = parser_config.instantiate(path=dataset_path, output_path=os.getcwd(), global_rank=0).get_outputs()
    return model, renderer, [camera.to_device(device) for camera in outputs.train_set.cameras]


def _save(path: str, vertices: Tensor, faces: Tensor, colors: Tensor):
    write_ply_mesh(path, vertices.cpu().numpy(), faces.cpu().numpy(), colors.cpu().numpy())
    print(f"mesh saved at {path}: {vertices.shape[0]} vertices, {faces.shape[0]} triangles")


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m gspl_amd.mesh", description="Extract a triangle mesh from a trained 2DGS model "
                                "(TSDF fusion of the rendered depth maps and marching tetrahedra, both on the GPU).")
    p.add_argument("model_path")
    p.add_argument("--dataset_path", default=None)
    p.add_argument("--voxel_size", type=float, default=-1.0)
    p.add_argument("--depth_trunc", type=float, default=-1.0)
    p.add_argument("--sdf_trunc", type=float, default=-1.0)
    p.add_argument("--num_cluster", type=int, default=50)
    p.add_argument("--unbounded", action="store_true")
    p.add_argument("--mesh_res", type=int, default=1024)
    return p


def main(argv: Optional[Sequence[str]] = None) -> None:
    args = parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("gspl_amd.mesh runs on the GPU only; there is no CPU fallback")
    device = torch.device("cuda")
    model, renderer, cameras = _load(args.model_path, args.dataset_path, device)
    model.active_sh_degree = 0          # diffuse colour only
    maps = render_views(model, renderer, cameras, torch.zeros(3, dtype=torch.float32, device=device))
    center, radius = estimate_bounding_sphere(cameras)
    print(f"bounding sphere: radius {radius:.2f} (use at least {2 * radius:.2f} for --depth_trunc)")
    if args.unbounded:
        name = "fuse_unbounded.ply"
        crop = min(512, args.mesh_res)
        vertices, faces, colors = extract_mesh_unbounded(maps, (center, radius), cameras, model, resolution=args.mesh_res, crop=crop)
    else:
        name = "fuse.ply"
        depth_trunc = radius * 2.0 if args.depth_trunc < 0 else args.depth_trunc
        voxel_size = depth_trunc / args.mesh_res if args.voxel_size < 0 else args.voxel_size
        sdf_trunc = 5.0 * voxel_size if args.sdf_trunc < 0 else args.sdf_trunc
        vertices, faces, colors = extract_mesh_bounded(maps, cameras, voxel_size, sdf_trunc, depth_trunc, center, radius)
    out_dir = args.model_path if os.path.isdir(args.model_path) else os.path.dirname(args.model_path)
    _save(os.path.join(out_dir, name), vertices, faces, colors)
    _save(os.path.join(out_dir, name.replace(".ply", "_post.ply")), *keep_largest_clusters(vertices, faces, args.num_cluster, colors=colors))


if __name__ == "__main__":
    main(sys.argv[1:])

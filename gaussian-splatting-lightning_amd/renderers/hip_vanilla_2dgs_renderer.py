"""HipVanilla2DGSRenderer — drop-in for the reference's `Vanilla2DGSRenderer` (internal/renderers/vanilla_2dgs_renderer.py:17-150), backed
by the HIP surfel rasterizer of ops/surfel.py instead of `diff_surfel_rasterization`.

Select with   --model.renderer gspl_amd.renderers.HipVanilla2DGSRenderer   (`--model.renderer.depth_ratio 1` for bounded
scenes, as the reference's option).  Outputs and `get_available_outputs` are the reference's: `render`, `viewspace_points` (its `.grad`
receives the 2DGS densification proxy), `visibility_filter`, `radii`, `rend_alpha`, `rend_normal` (world space), `view_normal`,
`rend_dist`, `surf_depth`, `surf_normal`.  By default the pseudo surface normal from the depth map stays in torch, on the camera's
device; with `--model.renderer.fused_maps true` everything after the rasterizer call is ONE HIP launch per direction
(`ops.surfel_maps`, csrc/normals.hip) with the camera's two 3x3 matrices kept on the camera object.  One difference of that route:
where alpha is 0 the gradient of the depth and alpha planes is 0 instead of the torch formulation's NaN.
"""
from __future__ import annotations

from typing import Dict

import torch

from .. import ops
from .renderer import Renderer, RendererOutputInfo, RendererOutputTypes, camera_hw, raster_settings


class HipVanilla2DGSRenderer(Renderer):
    def __init__(self, depth_ratio: float = 0., fused_maps: bool = False):
        super().__init__()
        self.depth_ratio = depth_ratio
        self.fused_maps = fused_maps

    def forward(self, viewpoint_camera, pc, bg_color: torch.Tensor, scaling_modifier=1.0, **kwargs):
        means3D = pc.get_xyz
        screenspace_points = torch.zeros_like(means3D, dtype=means3D.dtype, requires_grad=True, device=bg_color.device) + 0
        rasterizer = ops.SurfelGaussianRasterizer(raster_settings(viewpoint_camera, bg_color, scaling_modifier, pc.active_sh_degree,
                                                                  cls=ops.SurfelRasterizationSettings))
        colors_precomp = kwargs.get("colors_precomp", None)
        shs = pc.get_features if colors_precomp is None else None
        rendered_image, radii, allmap = rasterizer(means3D=means3D, means2D=screenspace_points, shs=shs, colors_precomp=colors_precomp,
                                                   opacities=pc.get_opacity, scales=pc.get_scaling[..., :2], rotations=pc.get_rotation,
                                                   cov3D_precomp=None)
        rets = {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0, "radii": radii}

        if self.fused_maps:
            normal_rot, rays = self.camera_matrices(viewpoint_camera, allmap)
            render_normal, surf_depth, surf_normal = ops.surfel_maps(allmap, normal_rot, rays, self.depth_ratio)
            rets.update({
                "rend_alpha": allmap[1:2],
                "rend_normal": render_normal,
                "view_normal": -allmap[2:5],
                "rend_dist": allmap[6:7],
                "surf_depth": surf_depth,
                "surf_normal": surf_normal,
            })
            return rets

        render_alpha = allmap[1:2]
        w2c3 = viewpoint_camera.world_to_camera[:3, :3].to(allmap.dtype)
        render_normal = (allmap[2:5].permute(1, 2, 0) @ w2c3.T).permute(2, 0, 1)      # view -> world space
        render_depth_median = torch.nan_to_num(allmap[5:6], 0, 0)
        render_depth_expected = torch.nan_to_num(allmap[0:1] / render_alpha, 0, 0)
        render_dist = allmap[6:7]
        surf_depth = render_depth_expected * (1 - self.depth_ratio) + self.depth_ratio * render_depth_median
        surf_normal = self.depth_to_normal(viewpoint_camera, surf_depth).permute(2, 0, 1)
        surf_normal = surf_normal * render_alpha.detach()
        rets.update({
            "rend_alpha": render_alpha,
            "rend_normal": render_normal,
            "view_normal": -allmap[2:5],
            "rend_dist": render_dist,
            "surf_depth": surf_depth,
            "surf_normal": surf_normal,
        })
        return rets

    @classmethod
    def camera_matrices(cls, view, like):
        """(normal_rot, rays) of `ops.surfel_maps` for a camera, [3, 3] each on `like`'s device: the view-to-world rotation of the
        normal planes and the matrix that takes (x, y, 1) to the pixel's ray, built with the torch expressions of `forward` and
        `depths_to_points` (no read-back) and kept on the camera object — dataset cameras persist across steps, so a step adds no
        matrix launches.  Keyed on identity and version counter of the two source tensors, as `GSplatV1.preprocess_camera`.  The op
        treats both as constants: the fused route passes no gradient to a camera pose."""
        dev, dt = like.device, like.dtype
        src = (view.world_to_camera, view.full_projection)
        cacheable = all(isinstance(v, torch.Tensor) and not v.requires_grad for v in src)
        if cacheable:
            key = tuple((id(v), v._version) for v in src) + camera_hw(view) + (str(dev), dt)
            hit = getattr(view, "_gspl_surfel_matrices", None)
            if hit is not None and hit[0] == key and all(a is b for a, b in zip(hit[1], src)):
                return hit[2], hit[3]
        w2c = view.world_to_camera.to(device=dev, dtype=dt)
        normal_rot = w2c[:3, :3].contiguous()
        c2w = w2c.T.inverse()
        W, H = camera_hw(view)
        ndc2pix = torch.tensor([[W / 2, 0, 0, W / 2], [0, H / 2, 0, H / 2], [0, 0, 0, 1]], dtype=dt, device=dev).T
        projection_matrix = c2w.T @ view.full_projection.to(device=dev, dtype=dt)
        intrins = (projection_matrix @ ndc2pix)[:3, :3].T
        rays = (c2w[:3, :3] @ intrins.inverse()).contiguous()
        if cacheable:
            try:
                view._gspl_surfel_matrices = (key, src, normal_rot, rays)
            except AttributeError:
                pass
        return normal_rot, rays

    @staticmethod
    def depths_to_points(view, depthmap):
        """World points of the depth map's pixels (pixel centres at integer coordinates), on the depth map's device."""
        dev, dt = depthmap.device, depthmap.dtype
        w2c = view.world_to_camera.to(device=dev, dtype=dt)
        c2w = w2c.T.inverse()
        W, H = camera_hw(view)
        ndc2pix = torch.tensor([[W / 2, 0, 0, W / 2], [0, H / 2, 0, H / 2], [0, 0, 0, 1]], dtype=dt, device=dev).T
        projection_matrix = c2w.T @ view.full_projection.to(device=dev, dtype=dt)
        intrins = (projection_matrix @ ndc2pix)[:3, :3].T
        grid_x, grid_y = torch.meshgrid(torch.arange(W, device=dev, dtype=dt), torch.arange(H, device=dev, dtype=dt), indexing="xy")
        points = torch.stack([grid_x, grid_y, torch.ones_like(grid_x)], dim=-1).reshape(-1, 3)
        rays_d = points @ intrins.inverse().T @ c2w[:3, :3].T
        rays_o = c2w[:3, 3]
        return depthmap.reshape(-1, 1) * rays_d + rays_o

    @classmethod
    def depth_to_normal(cls, view, depth):
        points = cls.depths_to_points(view, depth).reshape(*depth.shape[1:], 3)
        output = torch.zeros_like(points)
        dx = points[2:, 1:-1] - points[:-2, 1:-1]
        dy = points[1:-1, 2:] - points[1:-1, :-2]
        output[1:-1, 1:-1, :] = torch.nn.functional.normalize(torch.cross(dx, dy, dim=-1), dim=-1)
        return output

    def get_available_outputs(self) -> Dict:
        return {
            "rgb": RendererOutputInfo("render"),
            "render_alpha": RendererOutputInfo("rend_alpha", type=RendererOutputTypes.GRAY),
            "render_normal": RendererOutputInfo("rend_normal", type=RendererOutputTypes.NORMAL_MAP),
            "view_normal": RendererOutputInfo("view_normal", type=RendererOutputTypes.NORMAL_MAP),
            "render_dist": RendererOutputInfo("rend_dist", type=RendererOutputTypes.GRAY),
            "surf_depth": RendererOutputInfo("surf_depth", type=RendererOutputTypes.GRAY),
            "surf_normal": RendererOutputInfo("surf_normal", type=RendererOutputTypes.NORMAL_MAP),
        }

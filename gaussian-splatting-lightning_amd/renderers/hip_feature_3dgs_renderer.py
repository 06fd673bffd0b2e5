"""HipFeature3DGSRenderer — drop-in for the reference's `Feature3DGSRenderer`
(internal/renderers/feature_3dgs_renderer.py; configs/feature_3dgs/{sam,lseg,sam-speedup,lseg-speedup}.yaml) on the HIP ops:
same constructor, `setup` / `training_setup`, render types and output keys.

A trained, frozen model is projected under `no_grad`; the renderer owns one feature row per Gaussian (`self.features`, 128 / 256 /
512 wide, half of that in the speed-up mode, where a 1x1 convolution decodes the map) and distils a 2D foundation model's feature
maps into it.

Differences that are deliberate:
  * the feature map is ONE `ops.rasterize_features` call — one binning (shared with the RGB pass), one forward launch over all
    channels, and a backward that computes the feature gradient alone — where the reference loops over `rasterize_batch` channels
    at a time, each a full rasterization with a geometry backward nobody reads;
  * maps come out channels-first straight from the kernel;
  * `sklearn`, `viser` and `clip` are imported inside the methods that need them (the 2D PCA view, the viewer tab).
"""
from __future__ import annotations

from typing import Any, Dict

import torch

from .. import ops
from .renderer import Renderer, RendererOutputInfo, RendererOutputTypes, camera_hw, model_sh_pair
from .hip_gsplat_renderer import DEFAULT_BLOCK_SIZE, _project


class NoFeatureDecoder(torch.nn.Module):
    def forward(self, i):
        return i


class CNNDecoder(torch.nn.Module):
    """The speed-up mode's decoder: a 1x1 convolution from the rasterized width to the foundation model's."""

    def __init__(self, input_dim: int, output_dim: int, device=None):
        super().__init__()
        self.conv = torch.nn.Conv2d(input_dim, output_dim, kernel_size=1, device=device)

    def forward(self, x):
        return self.conv(x)


def pca_projection_matrix(features: torch.Tensor, n_components: int = 3, n_samples: int = 200_000, seed: int = 42) -> torch.Tensor:
    """[D, n_components]: the leading principal directions of a seeded sample of the rows (the D x D eigenproblem is solved on
    the host: a viewer path, run once per set of features)."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randint(0, features.shape[0], (n_samples,), generator=g).to(features.device)
    x = features[rows].float()
    x = x - x.mean(dim=0)
    _, vectors = torch.linalg.eigh((x.T @ x / x.shape[0]).cpu())      # ascending eigenvalues
    return vectors.flip(-1)[:, :n_components].contiguous().to(features.device)


def pca_colors(features: torch.Tensor, projection: torch.Tensor) -> torch.Tensor:
    colors = features @ projection
    colors = colors - colors.min(dim=0).values
    return colors / (colors.max(dim=0).values + 1e-6)


class HipFeature3DGSRenderer(Renderer):
    def __init__(self, speedup: bool, n_feature_dims: int, feature_lr: float = 0.001, feature_decoder_lr: float = 0.0001,
                 rasterize_batch: int = 32):
        """`rasterize_batch` is accepted for configuration compatibility and ignored: all channels are rasterized in one call."""
        super().__init__()
        self.speedup = speedup
        self.n_feature_dims = n_feature_dims
        self.feature_lr = feature_lr
        self.feature_decoder_lr = feature_decoder_lr
        self.rasterize_batch = rasterize_batch
        self.pca_projected_color = None      # of the current features; reset it when they change
        self.edit_mask = None                # [N] per-Gaussian mask of the "edited" view
        self.edit_mask_2d = None             # [h, w] mask applied to the RGB view

    def setup(self, stage: str, *args: Any, **kwargs: Any) -> Any:
        module = kwargs["lightning_module"]
        n_actual = self.n_feature_dims
        self.feature_decoder = NoFeatureDecoder()
        if self.speedup is True:
            n_actual = n_actual // 2
            self.feature_decoder = CNNDecoder(n_actual, self.n_feature_dims, device=module.device)
        self.n_actual_feature_dims = n_actual
        self.features = torch.nn.Parameter(torch.zeros((module.gaussian_model.n_gaussians, n_actual), dtype=torch.float,
                                                       device=module.device))

    def training_setup(self, module):
        optimizer = torch.optim.Adam(params=[
            {"name": "features", "params": [self.features], "lr": self.feature_lr},
            {"name": "feature_decoder", "params": self.feature_decoder.parameters(), "lr": self.feature_decoder_lr},
        ])
        return optimizer, None

    def forward(self, viewpoint_camera, pc, bg_color: torch.Tensor, scaling_modifier=1.0, render_types: list = None, **kwargs):
        if render_types is None:
            render_types = ["features"]
        W, H = camera_hw(viewpoint_camera)
        with torch.no_grad():
            xys, depths, radii, conics, comp, num_tiles_hit, _ = _project(
                pc.get_xyz, pc.get_scaling, pc.get_rotation, viewpoint_camera, scaling_modifier, DEFAULT_BLOCK_SIZE, W, H)
            opacities = pc.get_opacity * comp[:, None]      # anti-aliased
            # one sort for every pass that composites with `opacities`
            isects = ops.bin_gaussians(xys, depths, radii, H, W, DEFAULT_BLOCK_SIZE, conics=conics, opacities=opacities, lazy=True)

        def shared(opac):
            # other opacities than the binned ones (the "edited" view) bin for themselves
            return isects if opac is opacities else None

        def rasterize_rgb(colors, background, opac=opacities):
            return ops.rasterize_gaussians(xys, depths, radii, conics, num_tiles_hit, colors, opac, H, W, DEFAULT_BLOCK_SIZE,
                                           background=background, isects=shared(opac), channels_first=True)

        def view_colors():
            return ops.sh_view_colors(pc.active_sh_degree, pc.get_xyz, viewpoint_camera.camera_center, *model_sh_pair(pc), radii > 0,
                                      detach_means=True)

        outputs = {}
        if "rgb" in render_types:
            with torch.no_grad():
                outputs["render"] = rasterize_rgb(view_colors(), bg_color)
                if getattr(self, "edit_mask_2d", None) is not None:
                    mask = torch.nn.functional.interpolate(self.edit_mask_2d[None, None].float(), size=(H, W), mode="bilinear",
                                                           align_corners=True)[0]
                    outputs["render"] = outputs["render"] * (mask > 0.5)
        if "features" in render_types or "features_vanilla_pca_2d" in render_types:
            # every channel in one call, [D,H,W] from the kernel; the background of a feature map is zero
            raw_features = ops.rasterize_features(xys, depths, radii, conics, num_tiles_hit, self.features, opacities, H, W,
                                                  DEFAULT_BLOCK_SIZE, background=None, isects=isects, channels_first=True)
            outputs["raw_features"] = raw_features
            outputs["features"] = self.feature_decoder(raw_features)
        if "features_vanilla_pca_2d" in render_types:
            outputs["features_vanilla_pca_2d"] = self.feature_visualize(outputs["features"])
        if "features_pca_3d" in render_types:
            if getattr(self, "pca_projected_color", None) is None:
                with torch.no_grad():
                    normalized = torch.nn.functional.normalize(self.features, dim=-1)
                    normalized[torch.isnan(normalized)] = 0.
                    self.pca_projected_color = pca_colors(normalized, pca_projection_matrix(normalized))
            outputs["features_pca_3d"] = rasterize_rgb(self.pca_projected_color, bg_color)
        if "edited" in render_types:
            edited = opacities
            if getattr(self, "edit_mask", None) is not None:
                edited = opacities * self.edit_mask.unsqueeze(-1)
            outputs["edited"] = rasterize_rgb(view_colors(), bg_color, opac=edited)
        return outputs

    def training_forward(self, step: int, module, viewpoint_camera, pc, bg_color: torch.Tensor, scaling_modifier=1.0,
                         render_types: list = None, **kwargs):
        return self(viewpoint_camera=viewpoint_camera, pc=pc, bg_color=bg_color, scaling_modifier=scaling_modifier,
                    render_types=["features"], **kwargs)

    def get_available_outputs(self) -> Dict:
        return {
            "rgb": RendererOutputInfo(key="render"),
            "features": RendererOutputInfo(key="features", type=RendererOutputTypes.FEATURE_MAP),
            "features_vanilla_pca_2d": RendererOutputInfo(key="features_vanilla_pca_2d"),
            "features_pca_3d": RendererOutputInfo(key="features_pca_3d"),
            "edited": RendererOutputInfo(key="edited"),
        }

    def setup_web_viewer_tabs(self, viewer, server, tabs):
        self.viewer_options = ViewerOptions(self, viewer, server, tabs)

    @staticmethod
    def feature_visualize(feature: torch.Tensor) -> torch.Tensor:
        """[C,H,W] -> [3,H,W]: the first three principal components of every third pixel's normalised feature, scaled to the
        1st .. 99th percentile (needs scikit-learn)."""
        import numpy as np
        from sklearn.decomposition import PCA

        C, H, W = feature.shape
        flat = torch.nn.functional.normalize(feature, dim=0).permute(1, 2, 0).reshape(-1, C)
        samples = flat[::3].cpu().numpy()
        pca = PCA(3, random_state=42)
        transformed = pca.fit_transform(samples)
        mean = torch.tensor(samples.mean(0), dtype=torch.float, device=feature.device)
        components = torch.tensor(pca.components_, dtype=torch.float, device=feature.device)
        lo, hi = np.percentile(transformed, [1, 99])
        vis = ((flat - mean[None]) @ components.T - lo) / (hi - lo)
        return vis.clamp(0.0, 1.0).float().reshape(H, W, 3).permute(2, 0, 1)


class ViewerOptions:
    """The viewer's "Semantic" tab: with LSeg features (512 dims) a text query selects Gaussians for the "edited" view."""

    OBJECTS = ["car", "tree", "building", "sidewalk", "road"]

    def __init__(self, renderer: HipFeature3DGSRenderer, viewer, server, tabs):
        self.renderer, self.viewer, self.server, self.tabs = renderer, viewer, server, tabs
        with tabs.add_tab("Semantic"):
            if renderer.n_feature_dims == 512:
                self._lseg_options()
            else:
                server.gui.add_markdown("No option for SAM")

    def _encode_text(self, texts):
        import clip

        model, _ = clip.load("ViT-B/32", device=self.viewer.device)
        with torch.no_grad():
            encoded = model.float().encode_text(clip.tokenize(texts).to(self.viewer.device))
        del model
        torch.cuda.empty_cache()
        return encoded / encoded.norm(dim=-1, keepdim=True)

    @staticmethod
    def selection_score(features, queries, threshold, positive: int):
        """1 where a row's similarity to query `positive` passes `threshold`: (cosine + 1) / 2 against a single query, the softmax
        over the queries otherwise."""
        features = features / features.norm(dim=-1, keepdim=True)
        queries = queries / queries.norm(dim=-1, keepdim=True)
        scores = features.half() @ queries.T.half()
        if scores.shape[-1] == 1:
            return (((scores[:, 0] + 1.) / 2.) >= threshold).float()
        return (torch.nn.functional.softmax(scores, dim=-1)[:, positive] >= threshold).float()

    def _lseg_options(self):
        renderer, gui = self.renderer, self.server.gui
        text_features = self._encode_text([name.replace("_", " ") for name in self.OBJECTS])
        two_step = renderer.n_actual_feature_dims == 256      # speed-up mode: the Gaussians' rows are not in LSeg's space
        with gui.add_folder("LSeg"):
            chosen = gui.add_dropdown(label="Object", options=self.OBJECTS)
            score_2d = gui.add_slider(label="Score 2D", min=0., max=1., step=0.001, initial_value=1. / len(self.OBJECTS), visible=two_step)
            score_3d = gui.add_slider(label="Score 3D", min=0., max=1., step=0.001, initial_value=0.95 if two_step else 0.2)
            extract, reset = gui.add_button(label="Extract"), gui.add_button(label="Reset")
            gui.add_markdown("<b>[NOTE]</b> Switch to `edited` mode in 'General' panel to visualize the 3D extraction result")

        @extract.on_click
        def _(event):
            target = self.OBJECTS.index(chosen.value)
            with torch.no_grad(), self.server.atomic():
                if two_step:
                    # select pixels in the DECODED map of the current view, average their raw features, and select the Gaussians
                    # whose rows are close to that mean (objects outside the view are found poorly)
                    from internal.viewer.client import ClientThread
                    camera = ClientThread.get_camera(event.client.camera, self.viewer.max_res_when_moving.value).to_device(self.viewer.device)
                    out = renderer.forward(viewpoint_camera=camera, pc=self.viewer.viewer_renderer.gaussian_model,
                                           bg_color=torch.zeros((renderer.n_actual_feature_dims,), dtype=torch.float, device=self.viewer.device),
                                           render_types=["features"])
                    decoded = out["features"].permute(1, 2, 0)
                    mask_2d = self.selection_score(decoded.reshape(-1, renderer.n_feature_dims), text_features, score_2d.value, target) >= 0.5
                    mask_2d = mask_2d.reshape(decoded.shape[:2])
                    renderer.edit_mask_2d = mask_2d
                    mean_raw = out["raw_features"].permute(1, 2, 0)[mask_2d].reshape(-1, renderer.n_actual_feature_dims).mean(dim=0)
                    scores = self.selection_score(renderer.features, mean_raw[None], score_3d.value, 0)
                else:
                    scores = self.selection_score(renderer.features, text_features, score_3d.value, target)
                renderer.edit_mask = scores >= 0.5
            self.viewer.rerender_for_all_client()

        @reset.on_click
        def _(_):
            renderer.edit_mask = renderer.edit_mask_2d = None
            self.viewer.rerender_for_all_client()

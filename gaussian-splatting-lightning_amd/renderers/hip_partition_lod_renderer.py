"""HipPartitionLoDRenderer — the plugin for the reference's `PartitionLoDRenderer` (internal/renderers/partition_lod_renderer.py): a
frozen-model viewer and evaluation renderer over a scene cut into partitions, each trained at several levels of detail; every frame
picks one level per partition from the camera's distance (optionally dropping the partitions outside the view frustum) and renders
the chosen models as one.

Select with   --model.renderer gspl_amd.renderers.HipPartitionLoDRenderer --model.renderer.data <partition dir>
              --model.renderer.names "[fine, medium, coarse]"   (INTEGRATION.md).

The reference's per-frame front is torch ops, pytorch3d's box overlap, two host waits and, whenever the selection changes, a Python loop
over the partitions with one `.item()` each and five `torch.concat`; here it is `gspl_amd.lod.LoDSelector`: one `ops.lod_select`
launch, one 16-byte read, and one `ops.lod_gather` launch when the selection changed.  The frames themselves come from
`HipGSplatV1Renderer`, configured from the checkpoint's renderer hyper-parameters as the reference does.

The frustum test is an exact separating-axis test; the reference asks pytorch3d for an intersection volume > 1e-8.  The two differ for
solids that touch, and parity with pytorch3d's build is not pinned.

Not built (NotImplementedError): `partition_size` re-division, per-partition appearance models (`update_shs_dc`, the `LOD_SIDE`
switch), models that carry a Mip-Splatting 3D filter.  `setup()` follows the reference's directory layout through the reference's own
`PartitionTraining` and `GaussianModelLoader`; that loader path has not been run against real partition data — `from_table` is the
tested construction."""
from __future__ import annotations

import os
import time
from dataclasses import dataclass
from typing import Any, Dict, List

import torch

from ..lod import GatheredModel, LoDSelector, LoDTable
from .hip_gsplat_v1_renderer import GSplatV1, HipGSplatV1Renderer
from .renderer import Renderer, RendererConfig, RendererOutputInfo


@dataclass
class HipPartitionLoDRenderer(RendererConfig):
    data: str
    names: List[str]  # from finest to coarsest
    min_images: int = 32
    visibility_filter: bool = False
    freeze: bool = False
    drop_shs_rest: bool = False
    partition_size: float = None
    """Re-divide partitions (not built)"""

    lod_distances: List[int] = None
    """ i_distance = lod_distances[i] * default_partition_size, from finest to coarsest """

    ckpt_name: str = "preprocessed.ckpt"

    def instantiate(self, *args, **kwargs) -> "HipPartitionLoDRendererModule":
        if self.ckpt_name.endswith(".ckpt"):
            self.ckpt_name = self.ckpt_name[:self.ckpt_name.rfind(".")]
        level = os.environ.get("LOD_LEVEL", None)      # change at runtime: one level only
        if level is not None:
            level = int(level)
            self.names = self.names[level:level + 1]
            self.lod_distances = []
        if os.environ.get("LOD_SIDE", "") in ("left", "right"):
            raise NotImplementedError("HipPartitionLoDRenderer: LOD_SIDE selects checkpoints with retained appearance models; "
                                      "per-partition appearance models (`update_shs_dc`) are not built")
        if self.partition_size is not None:
            raise NotImplementedError("HipPartitionLoDRenderer: `partition_size` re-division (cutting the loaded partitions' models "
                                      "into a finer grid) is not built; leave it unset")
        return HipPartitionLoDRendererModule(self)


class HipPartitionLoDRendererModule(Renderer):
    MODEL_PROPERTIES = ["means", "shs", "opacities", "scales", "rotations"]

    def __init__(self, config: HipPartitionLoDRenderer) -> None:
        super().__init__()
        self.config = config
        self.synchronized = False
        self.on_render_hooks = []
        self.on_model_updated_hooks = []
        self.has_appearance_model = False
        self.table: LoDTable = None
        self.selector: LoDSelector = None
        self.gaussian_model: GatheredModel = None
        self.gsplat_renderer = None

    # ---- construction --------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_table(cls, table: LoDTable, box_min, box_max, thresholds=None, orientation_transform=None, corners=None,
                   default_partition_size: float = 1.0, config: HipPartitionLoDRenderer = None,
                   renderer_config: HipGSplatV1Renderer = None) -> "HipPartitionLoDRendererModule":
        """A module over a packed table.  box_min / box_max [P, 2] in the oriented frame, corners [P, 8, 3] in world space (needed by
        the visibility filter only), thresholds [L - 1] in scene units (default: the reference's (1 .. L - 1) x 0.25 x
        default_partition_size, or config.lod_distances x default_partition_size)."""
        config = config if config is not None else HipPartitionLoDRenderer(data=None, names=None)
        if config.partition_size is not None:
            raise NotImplementedError("HipPartitionLoDRenderer: `partition_size` re-division is not built; leave it unset")
        self = cls(config)
        self._attach(table, box_min, box_max, thresholds, orientation_transform, corners, default_partition_size,
                     renderer_config if renderer_config is not None else HipGSplatV1Renderer())
        return self

    def _attach(self, table, box_min, box_max, thresholds, orientation_transform, corners, default_partition_size, renderer_config,
                stage: str = "validate"):
        levels = table.n_levels
        self.default_partition_size = default_partition_size
        if thresholds is None:
            thresholds = torch.arange(1, levels, dtype=torch.float32) * 0.25 * default_partition_size
            if self.config.lod_distances is not None:
                distances = list(self.config.lod_distances)
                assert len(distances) == levels - 1 and all(a <= b for a, b in zip(distances, distances[1:])) and all(d >= 0 for d in distances)
                thresholds = torch.tensor(distances, dtype=torch.float32) * default_partition_size
        self.table = table
        self.selector = LoDSelector(table, box_min, box_max, thresholds, orientation_transform, corners)
        self.gaussian_model = GatheredModel(table)
        self.gsplat_renderer = renderer_config.instantiate()
        self.gsplat_renderer.setup(stage)

    def setup(self, stage: str, *args: Any, **kwargs: Any) -> Any:
        """The reference's loader (partition_lod_renderer.py:82-436) without re-division and appearance models: `partitions.pt`, then
        outputs/<lod>/<experiment>/<ckpt_name>.ckpt for every trainable partition of every level, through the reference's own
        `PartitionTraining` and `GaussianModelLoader`.  Not run against real partition data."""
        super().setup(stage, *args, **kwargs)
        if self.table is not None:
            return
        try:
            import internal  # noqa: F401
            import sys
            root = os.path.dirname(os.path.dirname(os.path.abspath(internal.__file__)))
            sys.path.insert(0, os.path.join(root, "utils"))
            from internal.utils.partitioning_utils import PartitionCoordinates
            from internal.utils.gaussian_model_loader import GaussianModelLoader
            from utils.train_partitions import PartitionTraining, PartitionTrainingConfig
        except ImportError as e:
            raise RuntimeError("HipPartitionLoDRenderer.setup loads partitions through the reference's `PartitionTraining` and "
                               "`GaussianModelLoader`; run inside the reference repository, or build the module with `from_table`") from e
        device = torch.device("cuda")
        partitions = torch.load(os.path.join(self.config.data, "partitions.pt"))
        transform = torch.eye(3)
        if partitions["extra_data"] is not None:
            transform = partitions["extra_data"]["rotation_transform"]
        transform = transform.T.to(device=device)[:3, :3].float()
        size = partitions["scene_config"]["partition_size"]
        coordinates = partitions["partition_coordinates"]
        if "size" not in coordinates:
            coordinates["size"] = torch.full((coordinates["xy"].shape[0], 2), size, dtype=torch.float, device=coordinates["xy"].device)
        coordinates = PartitionCoordinates(**coordinates)
        boxes = coordinates.get_bounding_boxes()

        levels, loaded, ckpt, model = [], None, None, None
        for lod in self.config.names:
            training = PartitionTraining(PartitionTrainingConfig(partition_dir=self.config.data, project_name=lod, min_images=self.config.min_images,
                                                                 n_processes=1, process_id=1, dry_run=False, extra_epoches=0))
            models, indices = [], []
            for index in training.get_trainable_partition_idx_list(min_images=self.config.min_images, n_processes=1, process_id=1):
                path = os.path.join(root, "outputs", lod, training.get_experiment_name(index), "{}.ckpt".format(self.config.ckpt_name))
                if not os.path.exists(path):
                    print("[WARNING]Checkpoint '{}.ckpt' of partition {} not found in {}".format(
                        self.config.ckpt_name, training.get_partition_id_str(index), lod))
                    continue
                ckpt = torch.load(path, map_location="cpu")
                model = GaussianModelLoader.initialize_model_from_checkpoint(ckpt, "cpu")
                model.pre_activate_all_properties()
                model.freeze()
                models.append(model)
                indices.append(index)
            if loaded is not None and indices != loaded:
                raise RuntimeError(f"HipPartitionLoDRenderer: level {lod} has checkpoints for partitions {indices}, the finest level for {loaded}")
            loaded = indices
            levels.append(models)
        if ckpt is None:
            raise RuntimeError(f"HipPartitionLoDRenderer: no '{self.config.ckpt_name}.ckpt' found for any partition of {self.config.names} "
                               f"under {os.path.join(root, 'outputs')}")
        table = LoDTable(levels, device=device, drop_shs_rest=self.config.drop_shs_rest)
        keep = torch.tensor(loaded)
        box_min, box_max = boxes.min[keep].to(device).float(), boxes.max[keep].to(device).float()

        # the partitions' 3-D boxes: the 2-D box between the 0.5 % and 99.5 % quantiles of the finest level's heights
        corners = []
        for p, fine in enumerate(levels[0]):
            z = fine.get_means().to(device) @ transform[:, -1:]
            lo, hi = torch.quantile(z, 0.005) - 1e-3, torch.quantile(z, 0.995) + 1e-3
            (x0, y0), (x1, y1) = box_min[p], box_max[p]
            ring = [(x0, y0), (x0, y1), (x1, y1), (x1, y0)]      # clockwise: left down, left top, right top, right down
            corners.append(torch.stack([torch.stack([x, y, h]) for h in (hi, lo) for x, y in ring]))
        corners = torch.stack(corners) @ transform.T
        hparams = ckpt["hyper_parameters"]["renderer"]
        renderer_config = HipGSplatV1Renderer(
            block_size=getattr(hparams, "block_size", 16), anti_aliased=getattr(hparams, "anti_aliased", True),
            filter_2d_kernel_size=getattr(hparams, "filter_2d_kernel_size", 0.3), separate_sh=getattr(hparams, "separate_sh", True),
            tile_based_culling=getattr(hparams, "tile_based_culling", False))
        self._attach(table, box_min, box_max, None, transform, corners, size, renderer_config, stage)

    # ---- the reference's attribute names ------------------------------------------------------------------------------------------
    lod_thresholds = property(lambda self: self.selector.thresholds)
    partition_lods = property(lambda self: self.selector.lod)
    is_partition_visible = property(lambda self: self.selector.visible)
    partition_distances = property(lambda self: self.selector.distance)

    def update_thresholds(self, values):
        self.selector.update_thresholds(values)

    def update_shs_dc(self, appearance_id):
        raise NotImplementedError("HipPartitionLoDRenderer: per-partition appearance models (`update_shs_dc`) are not built")

    def cuda_synchronize(self):
        if self.synchronized:
            return torch.cuda.synchronize()

    def forward(self, viewpoint_camera, pc, bg_color: torch.Tensor, scaling_modifier=1.0, render_types: list = None, **kwargs):
        """`pc` is not read: the model is the table's current selection, as in the reference."""
        if self.selector is None:
            raise RuntimeError("HipPartitionLoDRenderer: no partitions loaded (call setup(), or build the module with from_table)")
        self.cuda_synchronize()
        pipeline_started_at = appearance_updated_at = time.time()

        Ks, (width, height) = None, (0, 0)
        if self.config.visibility_filter:
            _, Ks, (width, height) = GSplatV1.preprocess_camera(viewpoint_camera)
        if self.selector.select(viewpoint_camera.camera_center, viewpoint_camera.world_to_camera if self.config.visibility_filter else None,
                                Ks, width, height, visibility_filter=self.config.visibility_filter, freeze=self.config.freeze):
            self.gaussian_model.properties = self.table.views()
            for hook in self.on_model_updated_hooks:
                hook()
        for hook in self.on_render_hooks:
            hook()
        self.cuda_synchronize()

        render_started_at = time.time()
        outputs = self.gsplat_renderer(viewpoint_camera, self.gaussian_model, bg_color, scaling_modifier, render_types, **kwargs)
        self.cuda_synchronize()
        finished_at = time.time()
        outputs["n_gaussians"] = self.gaussian_model.n_gaussians
        outputs["time"] = finished_at - pipeline_started_at
        outputs["render_time_with_lod_preprocess"] = finished_at - appearance_updated_at
        outputs["render_time"] = finished_at - render_started_at
        return outputs

    def get_available_outputs(self) -> Dict[str, RendererOutputInfo]:
        return self.gsplat_renderer.get_available_outputs()

    def setup_web_viewer_tabs(self, viewer, server, tabs):
        """The reference's "LoD" tab (partition_lod_renderer.py:666-733) without the per-partition labels: a Gaussian count, one
        "Max Distance" number per threshold, the visibility filter and freeze switches.  `server` is the viewer's viser server (only its `gui.add_*` are used; viser itself is
        not imported here)."""
        self.gsplat_renderer.setup_web_viewer_tabs(viewer, server, tabs)
        with tabs.add_tab("LoD"):
            with server.gui.add_folder("Status"):
                markdown = server.gui.add_markdown("")
            with server.gui.add_folder("Settings"):
                with server.gui.add_folder("Max Distance"):
                    numbers = [server.gui.add_number(label="LoD {}".format(i), initial_value=float(v))
                               for i, v in enumerate(self.selector.thresholds.tolist())]
                visibility = server.gui.add_checkbox("Visibility Filter", initial_value=self.config.visibility_filter)
                freeze = server.gui.add_checkbox("Freeze", initial_value=self.config.freeze)

        def thresholds_updated(_):
            self.update_thresholds([n.value for n in numbers])
            viewer.rerender_for_all_client()

        for number in numbers:
            number.on_update(thresholds_updated)

        @visibility.on_update
        def _(_):
            self.config.visibility_filter = visibility.value
            viewer.rerender_for_all_client()

        @freeze.on_update
        def _(_):
            self.config.freeze = freeze.value

        def count():
            markdown.content = "Gaussians: {}".format(self.gaussian_model.n_gaussians)

        self.on_model_updated_hooks.append(count)
        self._viewer_options = (markdown, numbers, visibility, freeze)

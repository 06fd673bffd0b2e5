"""The partition-LoD route without a GPU: the fp64 oracle tests/lod_oracle.py against the reference's own float64 run
(tests/golden/ref_lod.npz, made by tests/golden/make_lod_golden.py from `get_partition_distances`), its separating-axis visibility test
against an independent linear programme, the gather's 64-bit index helper built by the host compiler, table packing, the plugin's
config, pickling and viewer tab, and every refusal of `ops.lod_select` / `ops.lod_gather` that needs no device."""
import contextlib
import dataclasses
import os
import pickle
import subprocess
import types

import numpy as np
import pytest
import torch

import lod_oracle as LO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "ref_lod.npz")
BAND, BAND_CAP = 1e-6, 0.01


@pytest.fixture(scope="module")
def ref():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_oracle_matches_the_reference_run(ref):
    """Distances within 1e-12 of the reference's float64 run, and its levels exactly; the fixture has partitions at distance 0 (the
    camera above them) and every level chosen."""
    L = len(ref["thresholds"]) + 1
    for c, camera in enumerate(ref["cameras"]):
        d = LO.distances(camera, ref["transform"], ref["box_min"], ref["box_max"])
        assert d.shape == ref["distances"][c].shape and np.abs(d - ref["distances"][c]).max() <= 1e-12, c
        assert np.array_equal(LO.levels(ref["distances"][c], ref["thresholds"], L), ref["lods"][c]), c
    assert (ref["distances"] == 0).any() and set(np.unique(ref["lods"])) == set(range(L))


def test_separating_axes_agree_with_the_linear_programme():
    """600 random oriented boxes against the frustum of a 64 x 48 camera (fx = fy = 50, near 0.1, far 200): "no separating axis with a
    non-negative gap" and "Chebyshev radius of the 12 half-spaces > 0" agree wherever neither figure lies within 1e-6 of zero, and at
    most 1 % of the cases do."""
    rng = np.random.default_rng(7)
    F = LO.frustum(50.0, 50.0, 32.0, 24.0, 64, 48, far=200.0)
    inside_band = visible = 0
    for case in range(600):
        box = LO.random_box(rng)
        sep, radius = LO.separation(F, box), LO.chebyshev_radius(F, box)
        if abs(sep) <= BAND or abs(radius) <= BAND:
            inside_band += 1
            continue
        assert (sep < 0) == (radius > 0), (case, sep, radius)
        visible += sep < 0
    print(f"{visible} of 600 visible, {inside_band} within {BAND} of the boundary")
    assert inside_band <= BAND_CAP * 600 and 30 <= visible <= 570


def test_dst_start_and_gather_of_the_oracle():
    seg_start = np.array([0, 3, 3, 8, 10, 14, 15])      # L = 2, P = 3
    lod, visible = np.array([1, 0, 1]), np.array([True, True, False])
    assert LO.dst_start(lod, visible, seg_start, 3).tolist() == [0, 2, 2, 2]
    assert LO.dst_start(np.array([0, 1, 0]), np.ones(3, bool), seg_start, 3).tolist() == [0, 3, 7, 12]
    rows = np.arange(15)[:, None] * np.ones((1, 3))
    assert LO.gather(rows, np.array([0, 1, 0]), np.ones(3, bool), seg_start, 3)[:, 0].tolist() == [0, 1, 2, 10, 11, 12, 13, 3, 4, 5, 6, 7]
    assert LO.gather(rows, lod, np.zeros(3, bool), seg_start, 3).shape == (0, 3)


# ---- the index helper, by the host compiler ------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "gspl_lod_index.h"
int main(int argc, char** argv) {
    if (argc == 7) {
        const gspl::LodPiece p = gspl::lod_piece(atoll(argv[1]), atoll(argv[2]), atoll(argv[3]), atoi(argv[4]), atoll(argv[5]), atoll(argv[6]));
        printf("%lld %lld %lld %lld\n", (long long)p.src, (long long)p.dst, (long long)p.len, (long long)gspl::lod_row_of(atoll(argv[5]), atoi(argv[4])));
        return 0;
    }
    const int64_t starts[8] = {0, 5, 5, 9, 9, 9, 3000000000LL, 3000000007LL};      /* P = 7 */
    for (int i = 1; i < argc; ++i) printf("%d\n", gspl::lod_find_segment(starts, 7, atoll(argv[i])));
    return 0;
}
"""


@pytest.fixture(scope="module")
def helper(tmp_path_factory):
    d = tmp_path_factory.mktemp("lod_index")
    (d / "main.cpp").write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "gaussian-splatting-lightning_amd", "csrc"),
                           str(d / "main.cpp"), "-o", str(d / "lod_index")])
    return str(d / "lod_index")


def test_index_helper_at_three_billion_rows(helper):
    """Source and destination FLOAT offsets at R = 3 10^9 rows and K = 16 (width 48: 1.44 10^11 floats, 67 times 2^31) against Python's
    integers, for a window in the middle of a segment, one that starts before it and one that ends after it."""
    R, chunk = 3_000_000_000, 4096
    for width in (48, 3, 1, 4):
        src_begin, dst_begin, dst_end = R - 1000, R - 5000, R - 4000          # a 1000-row segment near the end of both arrays
        lo, hi = dst_begin * width, dst_end * width
        for f0 in (lo + 17 * width, lo - 100, hi - 50, (lo // chunk) * chunk):
            f1 = f0 + chunk
            d0, d1 = max(lo, f0), min(hi, f1)
            want = (src_begin * width + (d0 - lo), d0, d1 - d0, f0 // width)
            got = tuple(int(v) for v in subprocess.check_output([helper, *map(str, (src_begin, dst_begin, dst_end, width, f0, f1))], text=True).split())
            assert got == want, (width, f0)
            assert want[0] > 2 ** 31 or width == 1
    assert (R - 1000) * 48 > 2 ** 36


def test_segment_search_passes_over_empty_segments(helper):
    rows = [0, 4, 5, 8, 9, 2_999_999_999, 3_000_000_000, 3_000_000_006]
    got = [int(v) for v in subprocess.check_output([helper, *map(str, rows)], text=True).split()]
    assert got == [0, 0, 2, 2, 5, 5, 6, 6]


# ---- host-side behaviour ---------------------------------------------------------------------------------------------------------------
def _select_inputs(P=4, L=3, dtype=torch.float32):
    return dict(seg_start=torch.zeros(L * P + 1, dtype=torch.int64), camera_center=torch.zeros(3, dtype=dtype), transform=torch.eye(3, dtype=dtype),
                box_min=torch.zeros(P, 2, dtype=dtype), box_max=torch.ones(P, 2, dtype=dtype), thresholds=torch.ones(L - 1, dtype=dtype),
                prev_lod=torch.zeros(P, dtype=torch.int8), prev_visible=torch.ones(P, dtype=torch.uint8))


def test_select_refusals():
    from gspl_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lod_select(*_select_inputs().values())
    with pytest.raises(NotImplementedError, match="float32"):
        ops.lod_select(*_select_inputs(dtype=torch.float64).values())
    with pytest.raises(NotImplementedError, match="prev_lod must be int8"):
        ops.lod_select(*{**_select_inputs(), "prev_lod": torch.zeros(4, dtype=torch.int32)}.values())
    with pytest.raises(TypeError, match="camera_center must be a tensor"):
        ops.lod_select(*{**_select_inputs(), "camera_center": [0., 0., 0.]}.values())
    with pytest.raises(ValueError, match=r"thresholds must be \[2\], got \[3\]"):
        ops.lod_select(*{**_select_inputs(), "thresholds": torch.ones(3)}.values())
    with pytest.raises(ValueError, match=r"seg_start must be \[L \* 4 \+ 1\]"):
        ops.lod_select(*{**_select_inputs(), "seg_start": torch.zeros(11, dtype=torch.int64)}.values())
    with pytest.raises(ValueError, match="up to 65536 partitions"):
        ops.lod_select(*_select_inputs(P=65537, L=1).values())
    with pytest.raises(TypeError, match="boxes3d must be a tensor"):
        ops.lod_select(*_select_inputs().values(), visibility_filter=True)
    with pytest.raises(ValueError, match=r"boxes3d must be \[4, 8, 3\]"):
        ops.lod_select(*_select_inputs().values(), visibility_filter=True, boxes3d=torch.zeros(4, 8, 2), world_to_camera=torch.eye(4), Ks=torch.eye(3))


def _gather_inputs(R=10, K=4, P=2, L=2):
    return dict(seg_start=torch.zeros(L * P + 1, dtype=torch.int64), lod=torch.zeros(P, dtype=torch.int8), dst_start=torch.zeros(P + 1, dtype=torch.int64),
                n=5, means=torch.zeros(R, 3), shs=torch.zeros(R, K, 3), opacities=torch.zeros(R, 1), scales=torch.zeros(R, 3), rotations=torch.zeros(R, 4))


def test_gather_refusals():
    from gspl_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lod_gather(*_gather_inputs().values())
    with pytest.raises(NotImplementedError, match="shs must be float32"):
        ops.lod_gather(*{**_gather_inputs(), "shs": torch.zeros(10, 4, 3, dtype=torch.float16)}.values())
    with pytest.raises(ValueError, match=r"rotations must be \[10, 4\], got \[10, 3\]"):
        ops.lod_gather(*{**_gather_inputs(), "rotations": torch.zeros(10, 3)}.values())
    with pytest.raises(ValueError, match=r"n must be 0 \.\. 10"):
        ops.lod_gather(*{**_gather_inputs(), "n": 11}.values())
    with pytest.raises(TypeError, match="lod must be a tensor"):
        ops.lod_gather(*{**_gather_inputs(), "lod": None}.values())
    small = [torch.zeros(4, 3), torch.zeros(4, 4, 3), torch.zeros(4, 1), torch.zeros(4, 3), torch.zeros(4, 4)]
    with pytest.raises(ValueError, match=r"out means must be \[>= 5, 3\]"):
        ops.lod_gather(*_gather_inputs().values(), out=small)
    with pytest.raises(ValueError, match="five buffers"):
        ops.lod_gather(*_gather_inputs().values(), out=small[:4])


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """The C entry points themselves (include/gspl_hip.h section 26); none of these calls reaches the device."""
    import ctypes
    from gspl_amd import _lib as L
    lib = L.lib()
    block = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(block))

    def select(P=4, levels=3, thresholds=p, record=p, on=0, boxes=None):
        return lib.gspl_lod_select(P, levels, p, p, p, p, thresholds, boxes, None, None, 0, 0, on, p, p, p, p, p, p, p, record, None)

    def gather(P=4, levels=3, K=16, R=10, n=5, shs=p):
        return lib.gspl_lod_gather(P, levels, K, R, n, p, p, p, p, shs, p, p, p, p, p, p, p, p, None)

    bad = L.GSPL_ERR_INVALID_ARG
    assert select(P=0) == bad and select(P=65537) == bad and select(levels=0) == bad and select(levels=128) == bad
    assert select(thresholds=None) == bad and select(levels=1) == bad and select(record=None) == bad and select(on=1) == bad
    assert b"lod_select" in lib.gspl_last_error()
    assert gather(P=0) == bad and gather(levels=128) == bad and gather(K=0) == bad and gather(K=65) == bad and gather(n=11) == bad and gather(n=-1) == bad
    assert gather(shs=None) == bad and b"lod_gather" in lib.gspl_last_error()
    assert gather(n=0) == L.GSPL_OK and gather(n=0, shs=None) == L.GSPL_OK
    assert (L.GSPL_LOD_MAX_PARTITIONS, L.GSPL_LOD_MAX_LEVELS, L.GSPL_LOD_MAX_COEFFS) == (65536, 127, 64)


def _segment(n, K=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"means": torch.randn(n, 3, generator=g), "shs": torch.randn(n, K, 3, generator=g), "opacities": torch.rand(n, 1, generator=g),
            "scales": torch.rand(n, 3, generator=g), "rotations": torch.randn(n, 4, generator=g)}


def _levels(lengths, K=4):
    return [[_segment(n, K, seed=10 * l + p) for p, n in enumerate(level)] for l, level in enumerate(lengths)]


def test_table_packing():
    from gspl_amd.lod import LoDTable
    lengths = [[5, 0, 7], [3, 2, 1]]
    levels = _levels(lengths)
    table = LoDTable(levels, device="cpu")
    assert (table.n_levels, table.n_partitions, table.n_rows, table.n_coeffs, table.sh_degree) == (2, 3, 18, 4, 1)
    assert table.seg_start.tolist() == [0, 5, 5, 12, 15, 17, 18] and table.seg_start.dtype == torch.int64
    assert table.segment_length(0, 2) == 7 and table.segment_length(1, 1) == 2
    for k in ("means", "shs", "opacities", "scales", "rotations"):
        assert torch.equal(table.arrays[k][12:15], levels[1][0][k]) and table.arrays[k].shape[0] == 18 and table.arrays[k].is_contiguous()
    # the reference's drop_shs_rest: the DC coefficient alone, degree 0
    dropped = LoDTable(levels, device="cpu", drop_shs_rest=True)
    assert (dropped.n_coeffs, dropped.sh_degree) == (1, 0) and torch.equal(dropped.arrays["shs"][5:12], levels[0][2]["shs"][:, :1])
    # a model with separate shs_dc / shs_rest is packed as one array
    split = {**{k: v for k, v in levels[0][0].items() if k != "shs"}, "shs_dc": levels[0][0]["shs"][:, :1], "shs_rest": levels[0][0]["shs"][:, 1:]}
    assert torch.equal(LoDTable([[split]], device="cpu").arrays["shs"], levels[0][0]["shs"])
    # the destination buffers grow geometrically, never shrink, and hand out [:n] views
    first = table.reserve(4)
    assert table.capacity == 4 and table.reserve(3)[0] is first[0]
    assert table.reserve(5)[0].shape[0] == 8 and table.capacity == 8 and table.reserve(17)[0].shape[0] == 17 and table.reserve(2)[0].shape[0] == 17
    assert table.views(6)["shs"].shape == (6, 4, 3) and table.views(6)["means"].data_ptr() == table.reserve(1)[0].data_ptr()
    with pytest.raises(ValueError, match="every level must hold 3 partitions"):
        LoDTable([levels[0], levels[1][:2]], device="cpu")
    with pytest.raises(ValueError, match="rotations must be"):
        LoDTable([[{**levels[0][0], "rotations": torch.zeros(5, 3)}]], device="cpu")
    with pytest.raises(ValueError, match="lacks"):
        LoDTable([[{"means": torch.zeros(2, 3)}]], device="cpu")


def test_what_is_not_built_says_so(monkeypatch):
    from gspl_amd.lod import LoDTable
    from gspl_amd.renderers import HipPartitionLoDRenderer, HipPartitionLoDRendererModule
    seg = _segment(3)
    mip = types.SimpleNamespace(properties=seg, is_pre_activated=True, compute_3d_filter=lambda: None)
    with pytest.raises(NotImplementedError, match="3D filter"):
        LoDTable([[mip]], device="cpu")
    appearance = types.SimpleNamespace(properties=seg, is_pre_activated=True, get_appearance_features=lambda: None)
    with pytest.raises(NotImplementedError, match="appearance"):
        LoDTable([[appearance]], device="cpu")
    with pytest.raises(NotImplementedError, match="partition_size"):
        HipPartitionLoDRenderer(data="d", names=["a"], partition_size=50.).instantiate()
    table = LoDTable([[seg]], device="cpu")
    with pytest.raises(NotImplementedError, match="partition_size"):
        HipPartitionLoDRendererModule.from_table(table, torch.zeros(1, 2), torch.ones(1, 2), config=HipPartitionLoDRenderer(data="d", names=["a"], partition_size=1.))
    module = HipPartitionLoDRendererModule.from_table(table, torch.zeros(1, 2), torch.ones(1, 2))
    with pytest.raises(NotImplementedError, match="update_shs_dc"):
        module.update_shs_dc(3)
    monkeypatch.setenv("LOD_SIDE", "left")
    with pytest.raises(NotImplementedError, match="appearance"):
        HipPartitionLoDRenderer(data="d", names=["a"]).instantiate()
    with pytest.raises(ValueError, match="not pre-activated"):
        LoDTable([[types.SimpleNamespace(properties=seg, is_pre_activated=False)]], device="cpu")


def test_config_has_the_reference_fields_and_defaults(monkeypatch):
    """internal/renderers/partition_lod_renderer.py:21-35, written out: `data` and `names` are required, the rest defaults."""
    from gspl_amd import renderers
    fields = {f.name: f.default for f in dataclasses.fields(renderers.HipPartitionLoDRenderer)}
    assert fields == {"data": dataclasses.MISSING, "names": dataclasses.MISSING, "min_images": 32, "visibility_filter": False, "freeze": False,
                      "drop_shs_rest": False, "partition_size": None, "lod_distances": None, "ckpt_name": "preprocessed.ckpt"}
    assert list(fields) == ["data", "names", "min_images", "visibility_filter", "freeze", "drop_shs_rest", "partition_size", "lod_distances", "ckpt_name"]
    monkeypatch.delenv("LOD_LEVEL", raising=False)
    monkeypatch.delenv("LOD_SIDE", raising=False)
    cfg = renderers.HipPartitionLoDRenderer(data="scene", names=["fine", "medium", "coarse"], lod_distances=[1, 2])
    module = cfg.instantiate()
    assert isinstance(module, renderers.HipPartitionLoDRendererModule) and isinstance(module, renderers.Renderer) and module.config is cfg
    assert cfg.ckpt_name == "preprocessed" and cfg.names == ["fine", "medium", "coarse"] and cfg.lod_distances == [1, 2]
    assert module.MODEL_PROPERTIES == ["means", "shs", "opacities", "scales", "rotations"]
    # the LOD_LEVEL switch: that one level alone, no thresholds
    monkeypatch.setenv("LOD_LEVEL", "1")
    one = renderers.HipPartitionLoDRenderer(data="scene", names=["fine", "medium", "coarse"], lod_distances=[1, 2])
    one.instantiate()
    assert one.names == ["medium"] and one.lod_distances == []
    with pytest.raises(RuntimeError, match="no partitions loaded"):
        module(None, None, torch.zeros(3))


def test_config_and_module_are_picklable(monkeypatch):
    from gspl_amd import renderers
    monkeypatch.delenv("LOD_LEVEL", raising=False)
    cfg = renderers.HipPartitionLoDRenderer(data="scene", names=["a", "b"], visibility_filter=True)
    assert pickle.loads(pickle.dumps(cfg)) == cfg           # stored in checkpoint hparams by the reference
    assert pickle.loads(pickle.dumps(cfg.instantiate())).config == cfg


def test_default_thresholds_and_the_viewer_tab():
    """`setup_web_viewer_tabs` against a stand-in for the viser server: the inner renderer's tab, then "LoD" with one number per
    threshold, the two switches and the Gaussian count; the callbacks write the selector's thresholds and the config."""
    from gspl_amd.lod import LoDTable
    from gspl_amd.renderers import HipPartitionLoDRenderer, HipPartitionLoDRendererModule

    class Control:
        def __init__(self, label, initial_value=None):
            self.label, self.value, self.content, self.cb = label, initial_value, initial_value, None

        def on_update(self, fn):
            self.cb = fn
            return fn

    class Gui:
        def __init__(self):
            self.controls, self.folders = {}, []

        def _add(self, label, initial_value=None, **kw):
            self.controls[label] = Control(label, initial_value)
            return self.controls[label]

        def add_number(self, label, initial_value, **kw): return self._add(label, initial_value)
        def add_dropdown(self, label, initial_value, **kw): return self._add(label, initial_value)
        def add_checkbox(self, label, initial_value, **kw): return self._add(label, initial_value)
        def add_markdown(self, content): return self._add("markdown", content)

        def add_folder(self, name):
            self.folders.append(name)
            return contextlib.nullcontext()

    server = types.SimpleNamespace(gui=Gui())
    names, rerenders = [], []
    tabs = types.SimpleNamespace(add_tab=lambda name: names.append(name) or contextlib.nullcontext())
    viewer = types.SimpleNamespace(rerender_for_all_client=lambda: rerenders.append(1))

    table = LoDTable(_levels([[5, 6], [3, 2], [1, 1]]), device="cpu")
    module = HipPartitionLoDRendererModule.from_table(table, torch.zeros(2, 2), torch.ones(2, 2), default_partition_size=8.0)
    assert module.lod_thresholds.tolist() == [2.0, 4.0]                      # the reference's (1 .. L - 1) x 0.25 x partition size
    with_distances = HipPartitionLoDRendererModule.from_table(table, torch.zeros(2, 2), torch.ones(2, 2), default_partition_size=8.0,
                                                              config=HipPartitionLoDRenderer(data=None, names=None, lod_distances=[1, 3]))
    assert with_distances.lod_thresholds.tolist() == [8.0, 24.0]
    assert module.get_available_outputs().keys() == module.gsplat_renderer.get_available_outputs().keys() and "rgb" in module.get_available_outputs()
    assert module.partition_lods.tolist() == [127, 127] and module.is_partition_visible.tolist() == [1, 1]

    module.setup_web_viewer_tabs(viewer, server, tabs)
    gui = server.gui
    assert names == ["gsplat", "LoD"] and gui.folders == ["Status", "Settings", "Max Distance"]
    assert gui.controls["LoD 0"].value == 2.0 and gui.controls["LoD 1"].value == 4.0 and "Radius Clip" in gui.controls
    gui.controls["LoD 1"].value = 5.5
    gui.controls["LoD 1"].cb(None)
    assert module.lod_thresholds.tolist() == [2.0, 5.5] and len(rerenders) == 1
    gui.controls["Visibility Filter"].value = True
    gui.controls["Visibility Filter"].cb(None)
    gui.controls["Freeze"].value = True
    gui.controls["Freeze"].cb(None)
    assert module.config.visibility_filter is True and module.config.freeze is True
    table.reserve(4)
    module.gaussian_model.properties = table.views(4)
    for hook in module.on_model_updated_hooks:
        hook()
    assert gui.controls["markdown"].content == "Gaussians: 4"
    with pytest.raises(ValueError, match="2 thresholds"):
        module.update_thresholds([1.0])

"""No-GPU checks of the drop-in boundary: the ctypes binding is read from include/gspl_hip.h (the parser against literal C, the
widest signatures pinned, struct layouts against the C compiler), the C-ABI library loads and exports every symbol the header
declares, and the product path fails loudly instead of falling back (missing library, missing header, CPU tensors)."""
import ctypes
import os
import re
import subprocess
from ctypes import POINTER, c_char_p, c_float, c_int, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gspl_hip.h")

LITERAL_C = """
/* status codes ( a comment with gspl_ghost(int x), commas and = 3 */
enum { DEMO_OK = 0, DEMO_BAD = 7 /* seven (not 8), really */, DEMO_NEG = -1 };
#define GSPL_DEMO_FLOATS 12
typedef void* (*gspl_alloc_fn)(void* ctx, int tag, size_t bytes);   // NULL = failure
typedef struct gspl_demo_row { float* a; const float* b; float lr, beta; int32_t n; } gspl_demo_row;
typedef struct gspl_demo_state {
    int a, b, c;
    int64_t n;            /* the list length; see gspl_other( */
    float* p; uint8_t* q; uint32_t* r;
    uint32_t slots;
    gspl_demo_row first, second;
} gspl_demo_state;
size_t gspl_demo_bytes(int N, int64_t n);
const char* gspl_demo_name(void);
void* gspl_demo_stream(void);
int gspl_demo(int N, const float* x /* nullable */, int64_t n, uint64_t seed, float w, float* y,
              gspl_alloc_fn alloc, void* ctx, void* const* dst, const float* const* grads, void** out,
              gspl_demo_state* state, const gspl_demo_row* rows /* host array */, size_t bytes, void* stream);
"""


def test_parser_against_literal_c():
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib
    P = c_void_p
    constants, types, functions = _lib._parse_header(LITERAL_C)
    assert constants == {"DEMO_OK": 0, "DEMO_BAD": 7, "DEMO_NEG": -1, "GSPL_DEMO_FLOATS": 12}
    assert set(types) == {"gspl_alloc_fn", "gspl_demo_row", "gspl_demo_state"}
    Row, State, alloc = types["gspl_demo_row"], types["gspl_demo_state"], types["gspl_alloc_fn"]
    assert alloc is ctypes.CFUNCTYPE(P, P, c_int, c_size_t) and alloc is _lib.ALLOC_FN
    assert Row.__name__ == "DemoRow" and Row._fields_ == [("a", P), ("b", P), ("lr", c_float), ("beta", c_float), ("n", ctypes.c_int32)]
    assert State._fields_ == [("a", c_int), ("b", c_int), ("c", c_int), ("n", c_int64), ("p", P), ("q", P), ("r", P), ("slots", c_uint32),
                              ("first", Row), ("second", Row)]
    assert functions == {
        "gspl_demo_bytes": (c_size_t, [c_int, c_int64], ("N", "n")),
        "gspl_demo_name": (c_char_p, [], ()),
        "gspl_demo_stream": (c_void_p, [], ()),
        "gspl_demo": (c_int, [c_int, P, c_int64, c_uint64, c_float, P, alloc, P, P, P, P, POINTER(State), POINTER(Row), c_size_t, P],
                      ("N", "x", "n", "seed", "w", "y", "alloc", "ctx", "dst", "grads", "out", "state", "rows", "bytes", "stream")),
    }
    # a typed struct pointer takes byref / an array of THAT struct and refuses another one
    POINTER(Row).from_param((Row * 3)())
    POINTER(State).from_param(ctypes.byref(State()))
    with pytest.raises(TypeError):
        POINTER(State).from_param(ctypes.byref(Row()))


@pytest.mark.parametrize("declaration, named", [
    ("int gspl_bad(int N, double x);", "double x"),                        # an unknown type word: never c_void_p, never skipped
    ("int gspl_bad(int N, short* p);", "short* p"),                        # ... nor behind a pointer
    ("long gspl_bad(void);", "long"),                                      # ... nor as a return type
    ("int gspl_bad(int N, float);", "float"),                              # a parameter without a name
    ("static int gspl_counter;", "static int gspl_counter"),               # not a prototype
    ("typedef struct gspl_s { double d; } gspl_s;", "double d"),
    ("typedef struct gspl_s { float *a, *b; } gspl_s;", "float *a, *b"),   # declarator lists carry no pointers in this header
    ("enum { GSPL_X = 1 << 3 };", "GSPL_X = 1 << 3"),
    ("#define GSPL_X (1 + 2)", "GSPL_X (1 + 2)"),
    ("#pragma once", "#pragma once"),
])
def test_parser_refuses_what_it_cannot_classify(declaration, named):
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib
    with pytest.raises(_lib.HipLibraryError, match=re.escape(named)):
        _lib._parse_header("int gspl_fine(int N, void* stream);\n" + declaration + "\n")


def _declared():
    """The `gspl_name(` mentions outside block comments: found without the binding's parser, as a cross-check of its coverage."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gspl_\w+)\s*\(", src)))


def test_header_symbols_are_exported_and_bound():
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib
    declared = _declared()
    assert len(declared) >= 80
    assert declared == _lib.exported_symbols(), "the header parser misses or invents entry points"
    assert os.path.exists(_lib.LIB_PATH), "build the extension first: python -c 'import __graft_entry__ as g; g.build()'"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in gspl_hip.h but not exported"
    assert _lib.lib().gspl_abi_version() == _lib.ABI_VERSION == _lib.GSPL_ABI_VERSION == 39
    assert _lib.lib().gspl_last_error() is not None
    assert all(fn.restype is _lib._SIGNATURES[n][0] and fn.argtypes == _lib._SIGNATURES[n][1] for n in declared for fn in [getattr(_lib.lib(), n)])
    text = " ".join(re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S).split())
    assert "typedef void* (*gspl_alloc_fn)(void* ctx, int tag, size_t bytes);" in text
    assert _lib.ALLOC_FN is ctypes.CFUNCTYPE(c_void_p, c_void_p, c_int, c_size_t)


def test_widest_signatures_are_what_the_hand_kept_table_had():
    """The rows of the ctypes table this binding replaced, copied literally for the widest and most mixed entry points: the record
    that reading the header changed nothing."""
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib
    _P, ALLOC_FN, InriaState, SurfelState = c_void_p, _lib.ALLOC_FN, _lib.InriaState, _lib.SurfelState
    pinned = {
        "gspl_project_fwd": (c_int, [c_int, c_int, _P, _P, _P, _P, _P, c_int, c_int, c_int,
                                     c_float, c_float, c_float, c_float, c_float, c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
        "gspl_peer_wait": (c_int, [_P, c_int, ctypes.c_uint64, ctypes.c_uint64, _P, _P]),
        "gspl_rasterize_inria_fwd": (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_float, c_float, c_float,
                                             ALLOC_FN, _P, c_int64, _P, _P, ctypes.POINTER(InriaState), _P, _P]),
        "gspl_rasterize_surfel_bwd": (c_int, [c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, c_float, _P, ctypes.POINTER(SurfelState), _P, _P,
                                              ALLOC_FN, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
        "gspl_bilagrid_slice_bwd": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, c_int64, _P, c_int, _P, c_int, _P, c_int,
                                            _P, _P, c_int, _P, c_size_t, _P]),
    }
    for name, (restype, argtypes) in pinned.items():
        assert _lib._SIGNATURES[name][0] is restype, name
        assert _lib._SIGNATURES[name][1] == argtypes, name
    assert _lib._FUNCTIONS["gspl_rasterize_surfel_bwd"][2][16:18] == ("alloc_ctx", "v_rows")
    # the constants the table's module carried as literals
    assert (_lib.GSPL_RECORD_FLOATS, _lib.GSPL_BIN_SPAN_BYTES, _lib.GSPL_ADAM_MAX_TENSORS, _lib.GSPL_STATS_MAX_VIEWS) == (12, 64, 16, 16)
    assert (_lib.GSPL_INRIA_RAW_PARAMS, _lib.GSPL_INRIA_NO_SEGMENTS, _lib.GSPL_INRIA_FORCE_SEGMENTS, _lib.GSPL_INRIA_WILL_BACKWARD,
            _lib.GSPL_INRIA_PACKED_READY, _lib.GSPL_INRIA_ANTIALIAS, _lib.GSPL_INRIA_INVDEPTH) == (1, 2, 4, 8, 16, 32, 128)
    assert [getattr(_lib, "GSPL_BUF_" + n) for n in ("GEOMETRY", "BINNING", "IMAGE", "LISTS_WORK", "LISTS", "CHECKPOINTS", "PACKED",
                                                     "SURFEL_ENTRIES")] == [1, 2, 3, 4, 5, 6, 7, 8]
    assert _lib.CAMERA_MODELS == {"pinhole": 0, "ortho": 1, "fisheye": 2} and (_lib.GSPL_MODE_GSPLAT, _lib.GSPL_MODE_INRIA) == (0, 1)
    assert (_lib.GSPL_LAYOUT_HWC, _lib.GSPL_LAYOUT_CHW, _lib.GSPL_SH_ADD_HALF_CLAMP) == (0, 1, 1)
    assert (_lib.GSPL_INRIA_GEOMETRY, _lib.GSPL_INRIA_COLOURS, _lib.GSPL_INRIA_ALL) == (1, 2, 3)


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and every offsetof of the five structs as the host C compiler lays the header out, against the ctypes classes."""
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib
    structs = {"gspl_adam_tensor": _lib.AdamTensor, "gspl_bwd_adam_tensor": _lib.BwdAdamTensor, "gspl_bwd_adam_plan": _lib.BwdAdamPlan,
               "gspl_inria_state": _lib.InriaState, "gspl_surfel_state": _lib.SurfelState}
    assert {n for n, t in _lib._TYPES.items() if isinstance(t, type) and issubclass(t, ctypes.Structure)} == set(structs)
    lines = ['#include <stdio.h>', '#include "gspl_hip.h"', "int main(void) {"]
    for c_name, cls in structs.items():
        lines.append(f'    printf("{c_name} %zu\\n", sizeof({c_name}));')
        lines += [f'    printf("{c_name}.{field} %zu\\n", offsetof({c_name}, {field}));' for field, _ in cls._fields_]
    lines += ["    return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    measured = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    expected = {}
    for c_name, cls in structs.items():
        expected[c_name] = str(ctypes.sizeof(cls))
        expected.update({f"{c_name}.{field}": str(getattr(cls, field).offset) for field, _ in cls._fields_})
    assert len(expected) == 5 + 6 + 8 + 6 + 25 + 16 and measured == expected


def test_argument_errors_name_the_parameter(monkeypatch):
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib
    with pytest.raises(ctypes.ArgumentError, match=r"gspl_mcmc_reg_partials: argument 1 \(N\)"):
        _lib.call("gspl_mcmc_reg_partials", "three")
    with pytest.raises(ctypes.ArgumentError, match=r"gspl_peer_wait: argument 3 \(value\)"):
        _lib.call("gspl_peer_wait", None, 1, "x", 0, None, None)


def test_no_cpu_fallback():
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.spherical_harmonics(0, torch.zeros(4, 3), torch.zeros(4, 1, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.project_gaussians(torch.zeros(4, 3), torch.ones(4, 3), 1.0, torch.ones(4, 4), torch.eye(4), 100.0, 100.0, 50.0, 50.0, 100, 100, 16)


def test_missing_library_fails_loudly(monkeypatch):
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib
    monkeypatch.setattr(_lib, "_LIB", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libgspl_hip.so")
    with pytest.raises(_lib.HipLibraryError, match="only compute path"):
        _lib.lib()


def test_missing_header_fails_loudly():
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib
    assert os.path.samefile(_lib.HEADER_PATH, HEADER)
    with pytest.raises(_lib.HipLibraryError, match="binding of this package is read from it"):
        _lib._read_header("/nonexistent/include/gspl_hip.h")


def test_product_package_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "gaussian-splatting-lightning_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "import oracle" not in text and "from oracle" not in text and "gsplat_oracle" not in text, f


def test_renderer_plugins_importable_and_picklable():
    import pickle
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipGSplatRenderer, HipGSplatV1Renderer, HipVanillaRenderer, Renderer
    cfg = HipGSplatV1Renderer(block_size=16, anti_aliased=False)
    assert pickle.loads(pickle.dumps(cfg)) == cfg           # stored in checkpoint hparams by the reference
    mod = cfg.instantiate()
    assert isinstance(mod, Renderer) and isinstance(HipVanillaRenderer(), Renderer) and isinstance(HipGSplatRenderer(), Renderer)
    assert "rgb" in mod.get_available_outputs() and mod.parse_render_types(["rgb", "alpha"]) == 1 | 2 | 4
    from gspl_amd.renderers import GSplatV1
    culling = HipGSplatV1Renderer(tile_based_culling=True).instantiate()
    assert culling.isect_encode == GSplatV1.isect_encode_tile_based_culling and mod.isect_encode == GSplatV1.isect_encode_lists_only


def test_v1_renderer_viewer_tab_writes_the_runtime_options():
    """`setup_web_viewer_tabs` (Renderer plugin API, reference gsplat_v1_renderer.py:350-352,615-661) against a stand-in for the
    viser server: the two controls exist with the reference's labels and ranges, and their callbacks update `runtime_options`
    and ask for a re-render."""
    import contextlib
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import HipGSplatV1Renderer

    class Control:
        def __init__(self, **kw):
            self.kw, self.value, self.cb = kw, kw["initial_value"], None

        def on_update(self, fn):
            self.cb = fn
            return fn

    class Gui:
        def __init__(self):
            self.controls = {}

        def add_number(self, **kw):
            self.controls[kw["label"]] = Control(**kw)
            return self.controls[kw["label"]]

        def add_dropdown(self, **kw):
            self.controls[kw["label"]] = Control(**kw)
            return self.controls[kw["label"]]

    class Server:
        gui = Gui()

    class Tabs:
        names = []

        def add_tab(self, name):
            self.names.append(name)
            return contextlib.nullcontext()

    class Viewer:
        rerenders = 0

        def rerender_for_all_client(self):
            Viewer.rerenders += 1

    renderer = HipGSplatV1Renderer().instantiate()
    renderer.setup_web_viewer_tabs(Viewer(), Server(), Tabs())
    assert Tabs.names == ["gsplat"]
    clip, model = Server.gui.controls["Radius Clip"], Server.gui.controls["Camera Model"]
    assert clip.kw["min"] == 0. and clip.kw["max"] == 65535. and model.kw["options"] == ["pinhole", "ortho", "fisheye"]
    clip.value = 2.5
    clip.cb(None)
    model.value = "fisheye"
    model.cb(None)
    assert renderer.runtime_options.radius_clip == 2.5 and renderer.runtime_options.camera_model == "fisheye" and Viewer.rerenders == 2


def test_camera_scalars_are_read_once_per_camera_object_and_follow_changes():
    """`camera_scalars` keeps the python values of a camera's 0-d tensor fields on the camera object (the reference reads them
    with `.item()` on every call); a field replaced or modified in place is read again."""
    import types
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers.renderer import camera_hw, camera_scalars
    cam = types.SimpleNamespace(width=torch.tensor(640, dtype=torch.int32), height=torch.tensor(480, dtype=torch.int32),
                                fov_x=torch.tensor(0.75), idx=torch.tensor(7, dtype=torch.int32), plain=3)
    assert camera_hw(cam) == (640, 480) and all(isinstance(v, int) for v in camera_hw(cam))
    fov, idx, plain = camera_scalars(cam, ("fov_x", "idx", "plain"))
    assert fov == float(torch.tensor(0.75)) and idx == 7 and isinstance(idx, int) and plain == 3
    reads = {"n": 0}
    real_item = torch.Tensor.item

    def counting_item(self):
        reads["n"] += 1
        return real_item(self)
    torch.Tensor.item = counting_item
    try:
        assert camera_hw(cam) == (640, 480) and camera_scalars(cam, ("fov_x", "idx")) == (fov, 7)
        assert reads["n"] == 0                              # served from the object
        cam.width.fill_(800)                                # modified in place: version counter moves
        assert camera_hw(cam) == (800, 480) and reads["n"] == 1
        cam.height = torch.tensor(600, dtype=torch.int32)   # replaced
        assert camera_hw(cam) == (800, 600) and reads["n"] == 2
        assert camera_hw(cam) == (800, 600) and reads["n"] == 2
    finally:
        torch.Tensor.item = real_item

    class Slotted:                                          # an object that takes no new attributes: read every time, still right
        __slots__ = ("width", "height")
    s = Slotted()
    s.width, s.height = torch.tensor(32), torch.tensor(16)
    assert camera_hw(s) == (32, 16) and camera_hw(s) == (32, 16)


def test_v1_camera_constants_are_cached_per_camera_and_follow_edits():
    """`GSplatV1.preprocess_camera` keeps (view matrix, K) on the camera object; an in-place change of a source field, a replaced
    field, or a caller that edits the returned tensors in place all lead to a rebuild."""
    import types
    import gspl_amd  # noqa: F401
    from gspl_amd.renderers import GSplatV1
    cam = types.SimpleNamespace(world_to_camera=torch.eye(4), fx=torch.tensor(100.), fy=torch.tensor(101.), cx=torch.tensor(50.),
                                cy=torch.tensor(40.), width=torch.tensor(100), height=torch.tensor(80))
    a = GSplatV1.preprocess_camera(cam)
    b = GSplatV1.preprocess_camera(cam)
    assert a[0] is b[0] and a[1] is b[1] and a[2] == (100, 80)
    assert torch.equal(a[0][0], cam.world_to_camera.T) and float(a[1][0, 1, 1]) == 101.0 and float(a[1][0, 2, 2]) == 1.0
    b[1][0, 0, 2] -= 5.0                                     # a caller edits K in place
    c = GSplatV1.preprocess_camera(cam)
    assert c[1] is not b[1] and float(c[1][0, 0, 2]) == 50.0
    cam.fx.mul_(2)                                           # source modified in place
    assert float(GSplatV1.preprocess_camera(cam)[1][0, 0, 0]) == 200.0
    cam.world_to_camera = torch.eye(4) * 2                   # source replaced
    assert float(GSplatV1.preprocess_camera(cam)[0][0, 0, 0]) == 2.0
    pose = torch.eye(4, requires_grad=True)                  # a pose being optimised is never cached
    cam.world_to_camera = pose
    v = GSplatV1.preprocess_camera(cam)[0]
    assert v.requires_grad and GSplatV1.preprocess_camera(cam)[0] is not v
